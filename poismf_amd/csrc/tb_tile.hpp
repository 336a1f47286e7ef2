// tb_tile.hpp -- the users x items score tile shared by the batched top-N (topn_batch.hip) and the batched ranks (rank_batch.hip):
// a workgroup of four waves owns TB_TU = 64 rows of users (wave w: rows 16 w .. 16 w + 15) and walks the items TB_TJ = 64 at a time; the
// users' rows and the items' rows go through LDS in chunks of TB_KC columns, zero padded to a multiple of four columns.  tb_compute gives
// each (user, item) the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  -- fp32 on v_mfma_f32_16x16x4_f32, fp64
// on a VALU chain with the same register layout -- bit for bit what pair_dot_kernel (serve.hip) computes.  tb_walk is that walk with the
// items' rows and the kernel's epilogue as functors (tb_all_items: every item in order; topn_shared.hip: the items of a list); tb_excluded is the pair's one test "is item j in E(u)?".
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"

namespace {

constexpr int TB_WG = 256;                                // threads per workgroup (four waves)
constexpr int TB_TU = 64;                                 // users per workgroup
constexpr int TB_TJ = 64;                                 // items per step
constexpr int TB_KC = sizeof(real_t) == 4 ? 64 : 32;      // columns of the factors per LDS chunk
constexpr int TB_KS = TB_KC + 4;                          // LDS row stride (fp32: lanes (row l & 15, column l >> 4) fall on 64 distinct banks)
constexpr unsigned TB_NONE = 0xffffffffu;

typedef float tb_f32x4 __attribute__((ext_vector_type(4)));

// the total order: (s1, j1) comes before (s2, j2)
__device__ __forceinline__ bool tb_better(real_t s1, unsigned j1, real_t s2, unsigned j2) { return s1 > s2 || (s1 == s2 && j1 < j2); }

constexpr int TB_NL = TB_TU * TB_KC / TB_WG;   // elements of a [64 x TB_KC] tile per thread: element e = thread + i TB_WG is (row e / TB_KC, column e % TB_KC)

// rows [64 x TB_KC columns] of a row-major [* x k] factor into registers: columns c0 .. c0 + len - 1, zero elsewhere
template <class RowOf> __device__ __forceinline__ void tb_fetch(real_t (&v)[TB_NL], const real_t* src, int k, int c0, int len, RowOf row_of)
{
#pragma unroll
    for (int i = 0; i < TB_NL; i++) {
        const int e = (int)threadIdx.x + i * TB_WG;
        const int row = e / TB_KC, col = e % TB_KC;
        const long long r = row_of(row);   // < 0: no such row
        v[i] = 0;
        if (r >= 0 && col < len) v[i] = src[(size_t)r * (size_t)k + (size_t)(c0 + col)];
    }
}
__device__ __forceinline__ void tb_store(real_t* dst, const real_t (&v)[TB_NL])
{
#pragma unroll
    for (int i = 0; i < TB_NL; i++) {
        const int e = (int)threadIdx.x + i * TB_WG;
        dst[(e / TB_KC) * TB_KS + e % TB_KC] = v[i];
    }
}

// acc[t][r] += sum over the chunk's columns, in ascending order, of As[user][c] Bs[item][c] for user 16 wave + 4 (lane >> 4) + r and
// item 16 t + (lane & 15): one fused multiply-add per column
template <class T, bool MFMA> __device__ __forceinline__ void tb_compute(T (&acc)[4][4], const T* As, const T* Bs, int len)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned col = lane & 15, quad = lane >> 4;
    if constexpr (MFMA) {
#if defined(__HIP_DEVICE_COMPILE__)
        // A operand: user row (lane & 15), column 4 s + (lane >> 4); B operand: item row (lane & 15), same column;
        // D: item column lane & 15, user row 4 (lane >> 4) + register
        const int ksteps = (len + 3) / 4;
        const T* ap = As + (16 * wave + col) * TB_KS + quad;
        const T* bp = Bs + col * TB_KS + quad;
        tb_f32x4 d0 = { acc[0][0], acc[0][1], acc[0][2], acc[0][3] }, d1 = { acc[1][0], acc[1][1], acc[1][2], acc[1][3] };
        tb_f32x4 d2 = { acc[2][0], acc[2][1], acc[2][2], acc[2][3] }, d3 = { acc[3][0], acc[3][1], acc[3][2], acc[3][3] };
#pragma unroll 4
        for (int s = 0; s < ksteps; s++) {
            const float av = ap[4 * s];
            const float b0 = bp[4 * s], b1 = bp[16 * TB_KS + 4 * s], b2 = bp[32 * TB_KS + 4 * s], b3 = bp[48 * TB_KS + 4 * s];
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, d1, 0, 0, 0);
            d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2, d2, 0, 0, 0);
            d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3, d3, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { acc[0][r] = d0[r]; acc[1][r] = d1[r]; acc[2][r] = d2[r]; acc[3][r] = d3[r]; }
#endif
    } else {
        const T* ap = As + (16 * wave + 4 * quad) * TB_KS;
        const T* bp = Bs + col * TB_KS;
        for (int c = 0; c < len; c++) {
            T av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) av[r] = ap[r * TB_KS + c];
#pragma unroll
            for (int t = 0; t < 4; t++) bv[t] = bp[16 * t * TB_KS + c];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[t][r] = __builtin_fma(av[r], bv[t], acc[t][r]);
        }
    }
}

// The walk of one workgroup over the item tiles tile0 .. tile1 - 1: acc[t][r] = the whole chain for user 16 wave + 4 (lane >> 4) + r and the
// item of tile row 16 t + (lane & 15), then epilogue(acc, j_base), j_base = TB_TJ x the tile.  As / Bs: [TB_TU][TB_KS] each in LDS;
// user_row(row) is the tile row's row of A and item_row(j_base)(row) the tile row's row of B (< 0: none).
template <class T, bool MFMA, class UserRow, class ItemRow, class Epilogue>
__device__ __forceinline__ void tb_walk(T* As, T* Bs, const T* A, const T* B, int k, unsigned tile0, unsigned tile1, UserRow user_row,
                                        ItemRow item_row, Epilogue epilogue)
{
    static_assert(TB_TU == TB_TJ, "tb_fetch / tb_store serve both tiles");
    const int nchunks = (k + TB_KC - 1) / TB_KC;

    // k <= TB_KC: the users' tile is loaded once and the items' next tile travels in registers while this one is multiplied
    T b_next[TB_NL];
    if (nchunks == 1) {
        tb_fetch(b_next, A, k, 0, k, user_row);
        tb_store(As, b_next);
        tb_fetch(b_next, B, k, 0, k, item_row(tile0 * TB_TJ));
    }

    for (unsigned jt = tile0; jt < tile1; jt++) {
        const unsigned j_base = jt * TB_TJ;
        T acc[4][4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[t][r] = 0;
        if (nchunks == 1) {
            __syncthreads();   // every wave is done with the items' tile of the step before
            tb_store(Bs, b_next);
            __syncthreads();
            if (jt + 1 < tile1) tb_fetch(b_next, B, k, 0, k, item_row(j_base + TB_TJ));
            tb_compute<T, MFMA>(acc, As, Bs, k);
        } else {
            for (int ch = 0; ch < nchunks; ch++) {
                const int c0 = ch * TB_KC;
                const int len = k - c0 < TB_KC ? k - c0 : TB_KC;
                __syncthreads();   // every wave is done with the tiles of the step before
                tb_fetch(b_next, A, k, c0, len, user_row);
                tb_store(As, b_next);
                tb_fetch(b_next, B, k, c0, len, item_row(j_base));
                tb_store(Bs, b_next);
                __syncthreads();
                tb_compute<T, MFMA>(acc, As, Bs, len);
            }
        }
        epilogue(acc, j_base);
    }
}

// The items in order: tile row `row` of the step at j_base is item j_base + row, none from dimB on.
__device__ __forceinline__ auto tb_all_items(unsigned dimB)
{
    return [dimB](unsigned j_base) { return [dimB, j_base](int row) { const unsigned j = j_base + (unsigned)row; return j < dimB ? (long long)j : -1ll; }; };
}

// ---- "is item j in E(u)?" ----
struct TbExcl {
    const unsigned long long* seen_indptr;   // exclude_seen: the resident CSR (nullptr: off); local row = row of A - seen_row0
    const unsigned* seen_indices;
    unsigned seen_row0;
    int seen_sorted;                         // its rows are strictly ascending (binary search) or not known to be (scan)
    const unsigned* ex_indptr;               // the batch's own lists for this chunk (nullptr: none), strictly ascending rows
    const unsigned* ex_indices;
};

__device__ __forceinline__ bool tb_sorted_has(const unsigned* v, unsigned long long lo, unsigned long long hi, unsigned j)
{
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        const unsigned x = v[mid];
        if (x == j) return true;
        if (x < j) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// item j is in E(chunk user i, whose row of A is arow): the batch's list first, then the resident row
__device__ __forceinline__ bool tb_excluded(const TbExcl& x, unsigned i, unsigned arow, unsigned j)
{
    if (x.ex_indptr != nullptr && tb_sorted_has(x.ex_indices, x.ex_indptr[i], x.ex_indptr[i + 1], j)) return true;
    if (x.seen_indptr != nullptr) {
        const unsigned row = arow - x.seen_row0;
        const unsigned long long p0 = x.seen_indptr[row], p1 = x.seen_indptr[row + 1];
        if (x.seen_sorted) return tb_sorted_has(x.seen_indices, p0, p1, j);
        for (unsigned long long p = p0; p < p1; p++)
            if (x.seen_indices[p] == j) return true;
    }
    return false;
}

// ---- candidate lists in LDS: pruning and merging by rank counting under the total order (the batched top-N, dense and by include list) ----
constexpr int TB_PRUNE_Q = 3;                             // list entries per lane in a prune: lists hold <= 192 entries
constexpr size_t TB_MERGE_MAX = 2048;                     // entries of one user's partial lists the merge kernel ranks in LDS

__device__ __forceinline__ void tb_wave_sync()
{
    // LDS operations of one wave complete in order; this keeps the compiler from moving them across the point
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Rank-counts list `u` (c entries, c <= cap) under the total order, keeps the best min(c, n_top) in order and, when the list is full,
// sets the user's threshold to its last entry.  Called by a whole wave with uniform arguments.
__device__ __forceinline__ void tb_prune(real_t* ls, unsigned* li, unsigned c, unsigned n_top, unsigned* cnt_u, real_t* thr_s_u, unsigned* thr_j_u)
{
    const unsigned lane = threadIdx.x & 63;
    real_t es[TB_PRUNE_Q];
    unsigned ej[TB_PRUNE_Q], rk[TB_PRUNE_Q];
#pragma unroll
    for (int q = 0; q < TB_PRUNE_Q; q++) {
        const unsigned e = lane + 64u * q;
        es[q] = e < c ? ls[e] : (real_t)0;
        ej[q] = e < c ? li[e] : TB_NONE;
        rk[q] = 0;
    }
    for (unsigned i = 0; i < c; i++) {
        const real_t si = ls[i];
        const unsigned ji = li[i];
#pragma unroll
        for (int q = 0; q < TB_PRUNE_Q; q++) rk[q] += tb_better(si, ji, es[q], ej[q]) ? 1u : 0u;
    }
    tb_wave_sync();
#pragma unroll
    for (int q = 0; q < TB_PRUNE_Q; q++) {
        const unsigned e = lane + 64u * q;
        if (e < c && rk[q] < n_top) {
            ls[rk[q]] = es[q];
            li[rk[q]] = ej[q];
            if (rk[q] == n_top - 1) { *thr_s_u = es[q]; *thr_j_u = ej[q]; }
        }
    }
    if (lane == 0) *cnt_u = c < n_top ? c : n_top;
    tb_wave_sync();
}

// One wave: the best n_top of nslices sorted partial lists of n_top entries each (part_*: the first of them), by rank counting under the
// total order, to out_*[0 .. n_top); ranks no real entry reaches are left as they were.  ms / mj: TB_MERGE_MAX entries of LDS.
__device__ __forceinline__ void tb_merge_lists(real_t* ms, unsigned* mj, const real_t* part_score, const unsigned* part_ix, unsigned nslices,
                                               unsigned n_top, real_t* out_score, unsigned* out_ix)
{
    const unsigned lane = threadIdx.x;
    const unsigned m = nslices * n_top;
    for (unsigned i = lane; i < m; i += 64) { ms[i] = part_score[i]; mj[i] = part_ix[i]; }
    __syncthreads();
    for (unsigned e = lane; e < m; e += 64) {
        const real_t s = ms[e];
        const unsigned j = mj[e];
        if (j == TB_NONE) continue;
        // entries after e in its own (sorted) list are worse; empty entries (-inf, TB_NONE) are worse than every real one
        unsigned rk = e % n_top;
        const unsigned own = e / n_top;
        for (unsigned sl = 0; sl < nslices && rk < n_top; sl++) {
            if (sl == own) continue;
            for (unsigned i = sl * n_top; i < (sl + 1) * n_top; i++) {
                if (!tb_better(ms[i], mj[i], s, j)) break;   // (sorted: nothing further in this list is better either)
                rk++;
            }
        }
        if (rk < n_top) { out_score[rk] = s; out_ix[rk] = j; }
    }
}

// After tb_merge_lists, for a user that may have fewer than n_top real entries in all (a short row): the ranks none of them reached are
// marked empty (-inf, TB_NONE).  mj: the items tb_merge_lists left in LDS.
__device__ __forceinline__ void tb_merge_pad(const unsigned* mj, unsigned nslices, unsigned n_top, real_t* out_score, unsigned* out_ix)
{
    const unsigned lane = threadIdx.x;
    const unsigned m = nslices * n_top;
    unsigned real = 0;
    for (unsigned e0 = 0; e0 < m; e0 += 64) real += (unsigned)__popcll(__ballot(e0 + lane < m && mj[e0 + lane] != TB_NONE));
    for (unsigned i = real + lane; i < n_top; i += 64) {
        out_score[i] = (real_t)-__builtin_huge_val();   // -inf
        out_ix[i] = TB_NONE;
    }
}

}  // namespace
