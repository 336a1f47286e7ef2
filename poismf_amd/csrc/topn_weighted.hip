// topn_weighted.hip -- batched top-N with per-item score weights (include/poismf_hip.h, section 1o): section 1f's ranked list under
//
//   wscore(u, j) = score(u, j) * item_weight[j]     ONE multiplication rounded to real_t, after the chain and never fused into it
//   score(u, j)  = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t   (tb_tile.hpp)
//
// and the total order "wscore descending, then item index ascending".  The walk is tb_tile.hpp's and the selection -- the threshold
// test, the exclusion look-up, the append, the plain prune -- tb_select.hpp's, as in topn_batch.hip (topn_weighted_tile_kernel drives
// tb_walk with tb_all_items and TbSelect<T, TbPrunePlain>: a workgroup of four waves, 64 users, one slice of the items).  What differs
// is the epilogue: a lane holds the four users' scores against ONE item per pass (tb_compute's layout), so it loads that item's weight
// -- the four weights of a tile step up front, so that the loads are in flight together -- and multiplies its sixteen accumulators
// before they meet the threshold.  The selection then sees final scores only: its threshold, its prune and the merge of the slices'
// lists order them by a strict total order and assume nothing else about where a score came from, so pruning below the threshold and
// cutting the items into slices stay exact.  No LDS beyond the selection's.  No float atomics anywhere.
//
// A weight of 0 does not bar an item: it scores 0 and ties with its like by index.  A row may come out short (everything else is
// excluded): it is padded, by the tile kernel with one slice and by the merge otherwise.
//
// The host side converts nothing: the weights are real_t already, go up once per call in front of the chunk's parts, and the batch is
// cut into chunks of users as topn_quota.hip does (TwLayout; poismf_hip_topn_weighted_scratch_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"

namespace {

constexpr size_t TW_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many (topn_batch.hip's target)
constexpr size_t TW_MAX_ITEMS = POISMF_HIP_TOPN_WEIGHTED_MAX_ITEMS;
constexpr size_t TW_WEIGHTS_MAX = TW_MAX_ITEMS * sizeof(real_t);   // the weights at the item limit: 128 MiB in double
constexpr size_t TW_IDX_MAX = TW_MAX_ITEMS;               // exclusion indices a chunk may carry: any valid row fits (a row is shorter than dimB)
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, 0) <= TB_LDS_LIMIT, "the two tiles and 64 lists of the deepest n_top with TB_ROOM free slots fit LDS");
static_assert(TW_WEIGHTS_MAX + TW_IDX_MAX * sizeof(unsigned) + (32u << 20) <= TB_BUDGET, "the budget holds the weights, a chunk's exclusion lists and 32 MiB of lists");

struct TwArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users
    const real_t* weight;             // [dimB] item_weight
    real_t* part_score;               // [n_users][nslices][n_top]
    unsigned* part_ix;
};

// The one rounded multiplication of section 1o, written as the rounded-multiply intrinsic to name the intent.  What keeps it from being
// contracted is not the intrinsic (HIP's header may define it as a plain product) but the dataflow: -ffp-contract fuses a multiply INTO
// an add that consumes it, and this product is consumed by compares and stores only; its operand is a finished MFMA result (fp32) or
// the result of the chain's last fma (fp64), and fma(a, b, c) * w has no fused form.  Keep it that way: no add may take this product.
__device__ __forceinline__ float tw_mul(float s, float w) { return __fmul_rn(s, w); }
__device__ __forceinline__ double tw_mul(double s, double w) { return __dmul_rn(s, w); }

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void topn_weighted_tile_kernel(TwArgs a)
{
    extern __shared__ __align__(16) unsigned char tw_smem[];
    T* As = (T*)tw_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    const unsigned u_base = blockIdx.x * TB_TU;
    TbSelect<T, TbPrunePlain> sel;
    sel.init((unsigned char*)(Bs + TB_TJ * TB_KS), a.cap, a.n_top, TbPrunePlain(),
             [&](unsigned row) { return u_base + row < a.n_users ? a.users[u_base + row] : TB_NONE; });

    const unsigned ntiles = (a.dimB + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned col = threadIdx.x & 15;
    auto user_row = [&](int row) { return sel.user_row(row); };
    auto pos_of = [u_base](unsigned uu) { return u_base + uu; };   // a tile row's position in the chunk

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, tb_all_items(a.dimB), [&](T (&acc)[4][4], unsigned j_base) {
        // acc[t][r]: user 16 wave + 4 (lane >> 4) + r against item j_base + 16 t + col -- one weight per t
        T w[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            w[t] = j < a.dimB ? a.weight[j] : (T)0;
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[t][r] = tw_mul(acc[t][r], w[t]);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            sel.pass(acc[t], j, j < a.dimB, a.excl, pos_of);
        }
    });
    sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);   // (the best min(count, n_top), the rest marked empty)
}

// The one scratch allocation of a call, in bytes from the start: the weights, then what a chunk of users needs.  The chunk's parts are
// sized from what the budget leaves when the weights have their largest size, so that the layout of a chunk does not move with dimB.
struct TwLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t part_entries;     // (user, slice, rank) entries of the partial lists
    size_t weight, users, ex_indptr, ex_indices, part_score, part_ix, out_score, out_ix, total;
    // (user, slice) lists of a chunk of uc users: a slice per item tile at most and no more than the merge ranks in LDS; users x slices
    // <= TB_TU x (TW_TARGET_WGS + tiles)  (tb_slices)
    static size_t rows(size_t uc, size_t per_user_max) { return std::min(uc * per_user_max, TB_TU * TW_TARGET_WGS + TB_TU + uc); }
    TwLayout(size_t n_users, size_t n_top, size_t dimB)
    {
        const size_t E = sizeof(real_t) + sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), TW_MAX_ITEMS);
        const size_t slices_max = std::min(pmf_ceil_div(dimB, TB_TJ), std::max<size_t>(1, TB_MERGE_MAX / n_top));
        const size_t rest = TB_BUDGET - TW_WEIGHTS_MAX - TW_IDX_MAX * sizeof(unsigned) - 512;   // (512: alignment of the eight parts)
        // the largest chunk whose lists and results fit `rest`: either bound of rows() may be the one that lets it in
        const size_t uc_a = rest / (8 + (slices_max + 1) * n_top * E);
        const size_t fixed = (TB_TU * TW_TARGET_WGS + TB_TU) * n_top * E;
        const size_t uc_b = rest > fixed ? (rest - fixed) / (8 + 2 * n_top * E) : 0;
        size_t uc = std::min(std::max(uc_a, uc_b), TB_CHUNK_USERS_MAX);
        uc -= uc % TB_TU;                                                      // (>= TB_TU: uc_a is thousands at the deepest n_top in double)
        uc = std::min(uc, n_users);
        chunk_users = uc;
        idx_cap = std::min(TW_IDX_MAX, uc * dimB);                             // (no overflow: 2^18 x 2^24)
        part_entries = rows(uc, slices_max) * n_top;
        TbTake take;
        weight = take(dimB * sizeof(real_t));
        users = take(uc * sizeof(unsigned));
        ex_indptr = take((uc + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        part_score = take(part_entries * sizeof(real_t));
        part_ix = take(part_entries * sizeof(unsigned));
        out_score = take(uc * n_top * sizeof(real_t));
        out_ix = take(uc * n_top * sizeof(unsigned));
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_weighted_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k)
{
    (void)k;          // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TwLayout(n_users, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_weighted_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                   const real_t* item_weight, const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > TW_MAX_ITEMS || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || item_weight == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    for (size_t j = 0; j < dimB; j++)
        if (!std::isfinite(item_weight[j]) || item_weight[j] < (real_t)0) return 2;   // (-0 is 0)
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TW_IDX_MAX)) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_weighted_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                 const sparse_ix* users, size_t n_users, size_t n_top, const real_t* item_weight, PmfTopnSeen* seen,
                                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap,
                                 sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const TwLayout L(n_users, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, 0);
    const size_t lds = tb_lds_bytes(cap, 0);
    if (lds > TB_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the deepest n_top)
    auto kern = topn_weighted_tile_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));

    TB_TRY(pmf_upload(base + L.weight, item_weight, dimB * sizeof(real_t), stream));

    TwArgs a;
    std::vector<unsigned> hu, hp, hx, hix;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose exclusion lists fit the index area together
        // (a row is no longer than dimB, and the area holds min(TW_IDX_MAX, chunk x dimB): every row fits)
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, TW_TARGET_WGS, std::max<size_t>(1, TB_MERGE_MAX / n_top));   // (the merge kernel's LDS bounds them)
        const size_t nslices = sl.nslices;
        if (nu * nslices * n_top > L.part_entries) return 1;   // (cannot happen: TwLayout sizes the lists for any slicing of a chunk)
        a.A = dA;
        a.B = dB;
        a.users = (const unsigned*)(base + L.users);
        a.n_users = (unsigned)nu;
        a.dimB = (unsigned)dimB;
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.cap = (unsigned)cap;
        a.nslices = (unsigned)nslices;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        a.weight = (const real_t*)(base + L.weight);
        // (one slice: its sorted, padded lists are the results)
        a.part_score = (real_t*)(base + (nslices == 1 ? L.out_score : L.part_score));
        a.part_ix = (unsigned*)(base + (nslices == 1 ? L.out_ix : L.part_ix));
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            // the lists hold weighted scores already: the plain merge, padding the ranks a short row does not reach
            hipLaunchKernelGGL(topn_merge_kernel<true>, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, (unsigned)nu,
                               (unsigned)nslices, (unsigned)n_top, (real_t*)(base + L.out_score), (unsigned*)(base + L.out_ix));
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score), hix, out_ix, out_score, stream)) return 1;
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_weighted(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                             size_t n_top, const real_t* item_weight, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                             sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_weighted_check(users, n_users, n_top, dimA, dimB, (size_t)k, item_weight, excl_indptr, excl_indices)) return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_weighted_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, item_weight, nullptr,
                                                             excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
