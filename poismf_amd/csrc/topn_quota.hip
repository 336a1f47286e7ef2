// topn_quota.hip -- batched top-N with per-group quotas (include/poismf_hip.h, section 1n): section 1f's ranked list of every user, walked
// with one counter per group -- an item is taken iff fewer than q(g) items of its group were taken before it -- until n_top are taken.
//
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t   (tb_tile.hpp)
//
// The walk is tb_tile.hpp's and the selection -- the threshold test, the exclusion look-up, the append -- tb_select.hpp's, as in
// topn_batch.hip (topn_quota_tile_kernel drives tb_walk with tb_all_items and TbSelect: a workgroup of four waves, 64 users, one slice of
// the items, candidate lists of n_top + TB_ROOM + slack entries in LDS).  What differs is the prune, handed to the selection as its
// policy (tb_quota.hpp: TbPruneQuota, tb_prune_quota): an entry with q(g) entries of its
// own group before it dies, the rest are ranked among themselves, and the threshold is the n_top-th LIVE entry -- it exists only once
// n_top live entries do.  DESIGN.md section 4.19 has the argument why dropping below that threshold, and cutting the items into slices,
// stays exact.  The groups of a list's entries are staged per wave (TQ_STAGE words), not per user: 64 more arrays of `cap` words do not
// fit beside the lists at n_top = 128.  topn_quota_merge_kernel makes the same two counts over the union of a user's per-slice lists;
// with one slice the tile kernel writes the result rows itself.  No float atomics anywhere.
//
// Known slow path: where the quotas of the groups that have admissible items sum to less than n_top, n_top live entries never exist, the
// threshold never rises, every admissible item is a candidate and a list is pruned every pass or two.  The answer is right (and padded).
//
// The host side narrows the two maps to 32 bits per ITEM (group, and quota clipped to n_top), uploads them once per call in front of the
// chunk's parts, and cuts the batch into chunks of users as topn_batch.hip does (TqLayout; poismf_hip_topn_quota_scratch_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <type_traits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"
#include "tb_quota.hpp"

namespace {

constexpr size_t TQ_STAGE_BYTES = 4 * (size_t)TQ_STAGE * sizeof(unsigned);   // a group stage per wave, behind the selection in LDS
constexpr size_t TQ_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many (topn_batch.hip's target)
constexpr size_t TQ_MAX_ITEMS = POISMF_HIP_TOPN_QUOTA_MAX_ITEMS;
constexpr size_t TQ_MAPS_MAX = 2 * TQ_MAX_ITEMS * sizeof(unsigned);   // the two maps at the item limit: 128 MiB
constexpr size_t TQ_IDX_MAX = TQ_MAX_ITEMS;               // exclusion indices a chunk may carry: any valid row fits (a row is shorter than dimB)
static_assert(TB_N_TOP_MAX + TB_ROOM + 32 <= (size_t)TQ_STAGE, "a prune keeps a whole list in TB_PRUNE_Q registers per lane and its groups in the stage");
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, TQ_STAGE_BYTES) <= TB_LDS_LIMIT,
              "the two tiles, 64 lists of the deepest n_top with TB_ROOM free slots and four group stages fit LDS");
static_assert(TQ_MAPS_MAX + TQ_IDX_MAX * sizeof(unsigned) + (32u << 20) <= TB_BUDGET, "the budget holds the maps, a chunk's exclusion lists and 32 MiB of lists");

struct TqArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users
    const uint2* item_map;            // [dimB] (g(j), min(q(g(j)), n_top))
    real_t* part_score;               // [n_users][nslices][n_top]
    unsigned* part_ix;
};

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void topn_quota_tile_kernel(TqArgs a)
{
    extern __shared__ __align__(16) unsigned char tq_smem[];
    T* As = (T*)tq_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    unsigned char* sel_lds = (unsigned char*)(Bs + TB_TJ * TB_KS);
    unsigned* Gs = (unsigned*)(sel_lds + tb_select_bytes(a.cap));   // [4 waves][TQ_STAGE] groups of the list being pruned
    const unsigned u_base = blockIdx.x * TB_TU;
    TbSelect<T, TbPruneQuota> sel;
    sel.init(sel_lds, a.cap, a.n_top, TbPruneQuota{ Gs + (size_t)(threadIdx.x >> 6) * TQ_STAGE, a.item_map },
             [&](unsigned row) { return u_base + row < a.n_users ? a.users[u_base + row] : TB_NONE; });

    const unsigned ntiles = (a.dimB + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned col = threadIdx.x & 15;
    auto user_row = [&](int row) { return sel.user_row(row); };
    auto pos_of = [u_base](unsigned uu) { return u_base + uu; };   // a tile row's position in the chunk

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, tb_all_items(a.dimB), [&](T (&acc)[4][4], unsigned j_base) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            sel.pass(acc[t], j, j < a.dimB, a.excl, pos_of);
        }
    });
    sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);   // (the best min(live, n_top))
}

// One wave per user: the answer from its nslices sorted partial lists, [user][nslices][n_top].
__global__ __launch_bounds__(64) void topn_quota_merge_kernel(const real_t* part_score, const unsigned* part_ix, unsigned n_users, unsigned nslices,
                                                              unsigned n_top, const uint2* item_map, real_t* out_score, unsigned* out_ix)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX], mg[TB_MERGE_MAX], mq[TB_MERGE_MAX];
    __shared__ unsigned n_live;
    const unsigned u = blockIdx.x;
    if (u >= n_users) return;
    const size_t o = (size_t)u * nslices * n_top;
    tb_merge_lists_quota(ms, mj, mg, mq, &n_live, part_score + o, part_ix + o, nslices, n_top, item_map,
                         out_score + (size_t)u * n_top, out_ix + (size_t)u * n_top);
}

// The one scratch allocation of a call, in bytes from the start: the two maps, then what a chunk of users needs.  The chunk's parts are
// sized from what the budget leaves when the maps have their largest size, so that the layout of a chunk does not move with dimB.
struct TqLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t part_entries;     // (user, slice, rank) entries of the partial lists
    size_t item_map, users, ex_indptr, ex_indices, part_score, part_ix, out_score, out_ix, total;
    // (user, slice) lists of a chunk of uc users: a slice per item tile at most and no more than the merge ranks in LDS; users x slices
    // <= TB_TU x (TQ_TARGET_WGS + tiles)  (tb_slices)
    static size_t rows(size_t uc, size_t per_user_max) { return std::min(uc * per_user_max, TB_TU * TQ_TARGET_WGS + TB_TU + uc); }
    TqLayout(size_t n_users, size_t n_top, size_t dimB)
    {
        const size_t E = sizeof(real_t) + sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), TQ_MAX_ITEMS);
        const size_t slices_max = std::min(pmf_ceil_div(dimB, TB_TJ), std::max<size_t>(1, TB_MERGE_MAX / n_top));
        const size_t rest = TB_BUDGET - TQ_MAPS_MAX - TQ_IDX_MAX * sizeof(unsigned) - 512;   // (512: alignment of the nine parts)
        // the largest chunk whose lists and results fit `rest`: either bound of rows() may be the one that lets it in
        const size_t uc_a = rest / (8 + (slices_max + 1) * n_top * E);
        const size_t fixed = (TB_TU * TQ_TARGET_WGS + TB_TU) * n_top * E;
        const size_t uc_b = rest > fixed ? (rest - fixed) / (8 + 2 * n_top * E) : 0;
        size_t uc = std::min(std::max(uc_a, uc_b), TB_CHUNK_USERS_MAX);
        uc -= uc % TB_TU;                                                      // (>= TB_TU: uc_a is thousands at the deepest n_top in double)
        uc = std::min(uc, n_users);
        chunk_users = uc;
        idx_cap = std::min(TQ_IDX_MAX, uc * dimB);                             // (no overflow: 2^18 x 2^24)
        part_entries = rows(uc, slices_max) * n_top;
        TbTake take;
        item_map = take(dimB * 2 * sizeof(unsigned));
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

extern "C" size_t poismf_hip_topn_quota_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t n_groups, size_t k)
{
    (void)n_groups;   // (the maps are per item: a group's quota is written to each of its items)
    (void)k;          // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TqLayout(n_users, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_quota_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                const sparse_ix* group_of, size_t n_groups, const sparse_ix* quota, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > TQ_MAX_ITEMS || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || group_of == nullptr || quota == nullptr) return 2;
    if (n_groups == 0 || n_groups > 0x7fffffffull) return 2;   // (a group id is narrowed to 32 bits, and all bits set marks a dead entry)
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    for (size_t j = 0; j < dimB; j++)
        if ((size_t)group_of[j] >= n_groups) return 2;         // (a negative id of the R flavour is above every n_groups as a size_t)
    if (std::is_signed<sparse_ix>::value)
        for (size_t g = 0; g < n_groups; g++)
            if ((long long)quota[g] < 0) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TQ_IDX_MAX)) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_quota_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* group_of, size_t n_groups,
                              const sparse_ix* quota, PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                              void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score)
{
    (void)n_groups;
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const TqLayout L(n_users, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, TQ_STAGE_BYTES);
    const size_t lds = tb_lds_bytes(cap, TQ_STAGE_BYTES);
    if (lds > TB_LDS_LIMIT || cap > (size_t)TQ_STAGE) return 1;   // (cannot happen: the static_asserts above cover the deepest n_top)
    auto kern = topn_quota_tile_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));

    std::vector<unsigned> hu, hp, hx, hix;
    // the maps, per item, narrowed and interleaved: the group, and its quota clipped to n_top (n_top items of a group ahead: past the answer anyway)
    hx.resize(2 * dimB);
    for (size_t j = 0; j < dimB; j++) {
        hx[2 * j] = (unsigned)group_of[j];
        hx[2 * j + 1] = (unsigned)std::min<size_t>((size_t)quota[(size_t)group_of[j]], n_top);
    }
    TB_TRY(pmf_upload(base + L.item_map, hx.data(), 2 * dimB * sizeof(unsigned), stream));

    TqArgs a;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose exclusion lists fit the index area together
        // (a row is no longer than dimB, and the area holds min(TQ_IDX_MAX, chunk x dimB): every row fits)
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, TQ_TARGET_WGS, std::max<size_t>(1, TB_MERGE_MAX / n_top));   // (the merge kernel's LDS bounds them)
        const size_t nslices = sl.nslices;
        if (nu * nslices * n_top > L.part_entries) return 1;   // (cannot happen: TqLayout sizes the lists for any slicing of a chunk)
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
        a.item_map = (const uint2*)(base + L.item_map);
        // (one slice: its sorted lists are the results)
        a.part_score = (real_t*)(base + (nslices == 1 ? L.out_score : L.part_score));
        a.part_ix = (unsigned*)(base + (nslices == 1 ? L.out_ix : L.part_ix));
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            hipLaunchKernelGGL(topn_quota_merge_kernel, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, (unsigned)nu,
                               (unsigned)nslices, (unsigned)n_top, a.item_map, (real_t*)(base + L.out_score),
                               (unsigned*)(base + L.out_ix));
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score), hix, out_ix, out_score, stream)) return 1;
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_quota(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                          size_t n_top, const sparse_ix* group_of, size_t n_groups, const sparse_ix* quota, const sparse_ix* excl_indptr,
                          const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_quota_check(users, n_users, n_top, dimA, dimB, (size_t)k, group_of, n_groups, quota, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_quota_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, group_of, n_groups, quota,
                                                          nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
