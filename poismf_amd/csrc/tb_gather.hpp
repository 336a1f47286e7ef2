// tb_gather.hpp -- the ragged row gather one wave makes for 64 listed rows of B, shared by the batched top-N over include lists
// (topn_include.hip, section 1h) and the batched ranks over include lists (rank_include.hip, section 1j): lane l owns candidate l of
// the pass.  The 64 rows go through LDS in chunks of 256 bytes of a row.  All lanes load aligned 16-byte pieces, four neighbouring
// lanes one row's 64 consecutive bytes; rows start on sizeof(real_t) only, so a row's first and last piece carry up to 12 bytes of
// its neighbours (allocations of B carry 16 bytes of slack), which the copy into LDS drops: element by element to the row's own
// slot, 68 dwords apart, where each lane then reads its row 16 bytes at a time without bank conflicts.  The pieces of the next chunk
// (or pass) travel in registers (`pre`) while this one is multiplied.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "tb_tile.hpp"

namespace {

constexpr int TI_R = sizeof(real_t);
constexpr int TI_KC = 256 / TI_R;                         // columns of B per staged chunk: 256 bytes of a row
constexpr int TI_VN = 16 / TI_R;                          // elements of a 16-byte piece
constexpr int TI_SLOT = 256 + 16;                         // bytes between two rows of the LDS tile: 68 dwords = 4 x 17
constexpr int TI_NP_MAX = (256 + 16 - TI_R + 15) / 16;    // 16-byte pieces that cover 256 bytes starting anywhere on sizeof(real_t)
constexpr int TI_NI = 4 * ((TI_NP_MAX + 3) / 4);          // loads per lane and chunk: four lanes per row, sixteen rows per load
static_assert(TI_NP_MAX == 17 && TI_SLOT % 16 == 0 && (TI_SLOT / 16) % 2 == 1, "rows of the LDS tile: 16-byte aligned, 4 x odd dwords apart");

typedef unsigned ti_u32x4 __attribute__((ext_vector_type(4)));
typedef real_t ti_vec __attribute__((ext_vector_type(TI_VN)));

__device__ __forceinline__ float ti_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ti_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// One wave's gather: B as bytes, the wave's tile [64][TI_SLOT] in LDS, k, and this lane's part: it loads piece fq + 4 g of rows frow + 16 r.
struct TiGather {
    const char* Bb;
    unsigned char* Bs;
    int k;
    unsigned frow, fq;

    // the 16-byte pieces of columns c0 .. c0 + len - 1 of the rows jl (lane l: row l of the tile; TB_NONE: none) into `pre`
    __device__ __forceinline__ void fetch(ti_u32x4 (&pre)[TI_NI], unsigned jl, int c0, int len) const
    {
        const unsigned np = (unsigned)(len * TI_R + 16 - TI_R + 15) / 16;
        size_t byte0[4];
        bool has[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned jr = (unsigned)__shfl((int)jl, (int)(frow + 16 * r));
            has[r] = jr != TB_NONE;
            byte0[r] = ((size_t)jr * (size_t)k + (size_t)c0) * TI_R;
        }
#pragma unroll
        for (int i = 0; i < TI_NI; i++) {
            const int r = i & 3;
            const unsigned q = fq + 4 * (unsigned)(i >> 2);
            if (4 * (unsigned)(i >> 2) >= np) break;   // (uniform)
            const unsigned mis = (unsigned)(byte0[r] & 15);
            if (has[r] && 16 * q < mis + (unsigned)(len * TI_R))
                pre[i] = *(const ti_u32x4*)(Bb + (byte0[r] & ~(size_t)15) + 16 * (size_t)q);
        }
    }

    // `pre` into the tile: element by element, to column (its place in the row) of the row's slot; what belongs to a neighbouring row is dropped
    __device__ __forceinline__ void store(const ti_u32x4 (&pre)[TI_NI], unsigned jl, int c0, int len) const
    {
        const unsigned np = (unsigned)(len * TI_R + 16 - TI_R + 15) / 16;
        int shift[4];
        bool has[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned jr = (unsigned)__shfl((int)jl, (int)(frow + 16 * r));
            has[r] = jr != TB_NONE;
            shift[r] = (int)((((size_t)jr * (size_t)k + (size_t)c0) * TI_R) & 15) / TI_R;
        }
#pragma unroll
        for (int i = 0; i < TI_NI; i++) {
            const int r = i & 3;
            const unsigned q = fq + 4 * (unsigned)(i >> 2);
            if (4 * (unsigned)(i >> 2) >= np) break;   // (uniform)
            if (!has[r]) continue;
            real_t* dst = (real_t*)(Bs + (frow + 16 * r) * TI_SLOT);
            const ti_vec v = __builtin_bit_cast(ti_vec, pre[i]);
#pragma unroll
            for (int e = 0; e < TI_VN; e++) {
                const int cc = (int)q * TI_VN + e - shift[r];
                if (cc >= 0 && cc < len) dst[cc] = v[e];   // (a piece past the row's end was not loaded and has cc >= len)
            }
        }
    }
};

// The chain of one pass over a wave's 64 candidates (lane l: item j_cur, TB_NONE: none) through the gather: the score
// s = +0; for c in 0..k-1: s = fma(As[c], B[j_cur, c], s), with A's row As broadcast from LDS.  `pre` holds the first chunk of these
// rows on entry and, on return, the first chunk of the rows j_nxt when another pass follows (pass + 1 < npass).  This is the walk
// topn_include_kernel makes, statement for statement; that kernel keeps it written out, because routed through this function the
// compiler spills three more SGPRs there (26 against 23, both precisions) and its resource figures are to stay what they were.
__device__ __forceinline__ real_t ti_pass(const TiGather& g, ti_u32x4 (&pre)[TI_NI], const real_t* As, unsigned j_cur, unsigned j_nxt, unsigned pass,
                                          unsigned npass)
{
    const int k = g.k;
    const int nch = (k + TI_KC - 1) / TI_KC;
    const real_t* brow = (const real_t*)(g.Bs + (4 * g.frow + g.fq) * TI_SLOT);   // this lane's row of the tile
    real_t s = 0;
    for (int ch = 0; ch < nch; ch++) {
        const int c0 = ch * TI_KC;
        const int len = k - c0 < TI_KC ? k - c0 : TI_KC;
        tb_wave_sync();   // the wave is done with the tile of the step before
        g.store(pre, j_cur, c0, len);
        tb_wave_sync();
        {   // the step after this one: the next chunk of these rows, or the first chunk of the next pass's
            const bool same = ch + 1 < nch;
            const int n0 = same ? c0 + TI_KC : 0;
            if (same || pass + 1 < npass) g.fetch(pre, same ? j_cur : j_nxt, n0, k - n0 < TI_KC ? k - n0 : TI_KC);
        }
        if (j_cur != TB_NONE) {
            int c = 0;
            for (; c + TI_VN <= len; c += TI_VN) {
                const ti_vec av = *(const ti_vec*)(As + c0 + c);
                const ti_vec bv = *(const ti_vec*)(brow + c);
#pragma unroll
                for (int e = 0; e < TI_VN; e++) s = ti_fma(av[e], bv[e], s);
            }
            for (; c < len; c++) s = ti_fma(As[c0 + c], brow[c], s);
        }
    }
    return s;
}

}  // namespace
