// topn_adjust.hip -- batched top-N with per-(user, item) score factors (include/poismf_hip.h, section 1r): section 1f's ranked list under
//
//   ascore(u, j) = score(u, j) * f(u, j)   where (u, j) is listed in the user's adjust row: ONE multiplication rounded to real_t, after
//                                          the chain and never fused into it (ta_mul);  score(u, j) untouched otherwise
//   score(u, j)  = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t   (tb_tile.hpp, tb_gather.hpp)
//
// and the total order "ascore descending, then item index ascending".  A factor may exceed 1, so a listed cell cannot be found only
// after the threshold test, and a look-up per score in the tile's epilogue would put a binary search on every one of users x items
// scores.  Hence two stages and a merge:
//   dense    topn_adjust_tile_kernel: topn_batch.hip's walk (tb_walk, tb_all_items) and selection (TbSelect<T, TbPrunePlain>) over all
//            items, with the user's listed cells treated as excluded -- the host stages the chunk's exclusion rows as the union of the
//            caller's row and the adjust row's indices, so tb_excluded and TbSelect::pass are what they were.  Sorted partial lists
//            per (user, item slice).
//   sparse   topn_adjust_sparse_kernel: one wave per (user, slice of its adjust row), planned on the host as topn_include.hip plans
//            its work items.  The listed rows of B go through the gather of tb_gather.hpp (ti_pass), lane l owning cell l of the
//            pass; the lane multiplies its finished score by its cell's factor -- loaded next to the index, so that both are in flight
//            together -- and the include kernel's selection follows: a threshold in LDS, an append through an integer LDS counter,
//            tb_prune when fewer than 64 slots are free.  The host has removed the cells of the caller's exclusion row from the adjust
//            row, so a survivor is looked up in the resident exclude_seen row only.  Sorted partial lists of n_top entries, padded.
//   merge    topn_adjust_merge_kernel: one wave per user ranks its dense and sparse lists together (tb_merge_lists) and pads what no
//            entry reaches (tb_merge_pad).  A user's lists lie side by side from a first row of its own (topn_include.hip's ragged
//            merge): the dense slices, then its sparse slices -- TbSelect::finish takes the row from that table, so a long row costs
//            the other users of its chunk nothing.  The items of the two stages are disjoint, so the strict total order needs nothing
//            new.  A chunk without a listed cell is section 1f's: one slice writes the result rows, several go through
//            topn_merge_kernel.
// No float atomics anywhere.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a
// chunk's users, united exclusion rows, adjust cells (index and factor), work items, partial lists and results (TaLayout;
// poismf_hip_topn_adjusted_scratch_bytes reports its size).  The united rows are built per chunk, never for the whole batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"

namespace {

constexpr size_t TA_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many (topn_batch.hip's target)
constexpr int TA_WAVES = 4;                               // work items of the sparse stage per workgroup
constexpr unsigned TA_CAP = (unsigned)TB_N_TOP_MAX + 64;  // slots of a wave's candidate list: a pass can add 64
constexpr size_t TA_SLICE_MIN = 1024;                     // cells per work item, unless the merge's LDS asks for more
constexpr size_t TA_MAX_ITEMS = POISMF_HIP_TOPN_ADJUSTED_MAX_ITEMS;
constexpr size_t TA_MAX_ROW = POISMF_HIP_TOPN_ADJUSTED_MAX_ROW;
constexpr size_t TA_IDX_MAX = TA_MAX_ITEMS;               // exclusion indices a chunk may carry: any united row fits (it is no longer than dimB)
constexpr size_t TA_CELL = sizeof(unsigned) + sizeof(real_t);   // an adjust cell on the device: index and factor
static_assert(TA_CAP <= (unsigned)TB_PRUNE_Q * 64, "a prune keeps a whole list in TB_PRUNE_Q registers per lane");
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, 0) <= TB_LDS_LIMIT, "the two tiles and 64 lists of the deepest n_top with TB_ROOM free slots fit LDS");
static_assert(TA_IDX_MAX * sizeof(unsigned) + TA_MAX_ROW * TA_CELL + (64u << 20) <= TB_BUDGET,
              "the budget holds a full exclusion area, the longest adjust row and 64 MiB of users, work items, lists and results");

// lists of one user the merge ranks in LDS, and how the two stages share them
inline size_t ta_lists_max(size_t n_top) { return std::max<size_t>(2, TB_MERGE_MAX / n_top); }
inline size_t ta_dense_max(size_t n_top) { return ta_lists_max(n_top) / 2; }
inline size_t ta_sparse_max(size_t n_top) { return ta_lists_max(n_top) - ta_dense_max(n_top); }
// cells per work item of an adjust row of len cells, and its work items
inline size_t ta_slice(size_t len, size_t n_top) { return pmf_round_up(std::max(TA_SLICE_MIN, pmf_ceil_div(len, ta_sparse_max(n_top))), 64); }
inline size_t ta_slices_of(size_t len, size_t n_top) { return len ? pmf_ceil_div(len, ta_slice(len, n_top)) : 0; }
// ta_slices_of is NOT monotone in len (the slice is rounded up to 64: at n_top = 10 a row of 104449 cells has 97 work items, one of
// 104448 has 102), and a row loses the cells its user's exclusion row holds after the chunk was cut.  What the cut charges a row is
// this bound instead: it never decreases with len and is no less than the work items of any row of at most len cells (a slice is at
// least TA_SLICE_MIN cells, and no row has more than ta_sparse_max work items)
inline size_t ta_slices_bound(size_t len, size_t n_top) { return len ? std::min(ta_sparse_max(n_top), len / TA_SLICE_MIN + 1) : 0; }

// The one rounded multiplication of section 1r (topn_weighted.hip's tw_mul, and its reasoning): the product is consumed by compares and
// stores only, and its operand is the finished chain, so nothing can contract it.  Keep it that way: no add may take this product.
__device__ __forceinline__ float ta_mul(float s, float f) { return __fmul_rn(s, f); }
__device__ __forceinline__ double ta_mul(double s, double f) { return __dmul_rn(s, f); }

// ---- dense stage ----
struct TaDenseArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) united with the adjust row, of the chunk's users
    const unsigned* first;            // TABLE: [n_users + 1] a user's first row of the partial lists: its item slices, then its sparse slices
    real_t* part_score;               // [rows][n_top]; without the table user i's rows are i x nslices on, as in topn_batch.hip
    unsigned* part_ix;
};

// TABLE: something is listed in the chunk and the users' rows come from a.first.  Without it the kernel is topn_tile_kernel, statement
// for statement (the table's pointer, kept for finish, costs eleven more SGPRs spilled across the item loop: DESIGN.md section 4.23)
template <class T, bool MFMA, bool TABLE> __global__ __launch_bounds__(TB_WG) void topn_adjust_tile_kernel(TaDenseArgs a)
{
    extern __shared__ __align__(16) unsigned char ta_smem[];
    T* As = (T*)ta_smem;                                  // [TB_TU][TB_KS]
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
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            sel.pass(acc[t], j, j < a.dimB, a.excl, pos_of);
        }
    });
    // (the best min(count, n_top), the rest marked empty) to the user's row of this item slice
    if constexpr (TABLE) sel.finish(a.part_score, a.part_ix, 1u, blockIdx.y, [&](unsigned uu) { return a.first[u_base + uu]; });
    else sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);
}

// ---- sparse stage ----
struct TaItem { unsigned ui, p0, len, dst; };             // chunk user, first cell in the chunk's adjust area, cells, row of the partial lists

struct TaSparseArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    const TaItem* items;
    unsigned n_items;
    const unsigned* adj_ix;           // the chunk's adjust rows, one after the other, without the cells of the caller's exclusion rows
    const real_t* adj_f;              // their factors
    int k;
    unsigned n_top;
    TbExcl excl;                      // the resident rows only (exclude_seen)
    real_t* part_score;               // [partial rows][n_top]
    unsigned* part_ix;
};

__host__ __device__ inline size_t ta_wave_lds(size_t k)
{
    const size_t ka = (k + 3) & ~(size_t)3;
    return (64 * (size_t)TI_SLOT + (ka + TA_CAP + 1) * TI_R + (TA_CAP + 2) * sizeof(unsigned) + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(64 * TA_WAVES) void topn_adjust_sparse_kernel(TaSparseArgs a)
{
    extern __shared__ __align__(16) unsigned char ta_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned item = blockIdx.x * TA_WAVES + wave;
    if (item >= a.n_items) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.k;
    const int ka = (k + 3) & ~3;
    unsigned char* Bs = ta_smem + wave * ta_wave_lds((size_t)k);   // [64][TI_SLOT]: the pass's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                     // [ka] the user's row, zero padded
    real_t* Ls = As + ka;                                          // [TA_CAP] candidate scores
    real_t* thr_s = Ls + TA_CAP;                                   // threshold: score ...
    unsigned* Li = (unsigned*)(thr_s + 1);                         // [TA_CAP] candidate items
    unsigned* thr_j = Li + TA_CAP;                                 // ... and item
    unsigned* cnt = thr_j + 1;                                     // entries in the list

    const TaItem it = a.items[item];
    const unsigned arow = a.users[it.ui];
    const real_t* Au = a.A + (size_t)arow * (size_t)k;
    for (int c = (int)lane; c < ka; c += 64) As[c] = c < k ? Au[c] : (real_t)0;
    // the threshold starts as the empty entry (-inf, TB_NONE): every real (s, j), a score of -inf included, beats it
    if (lane == 0) { *thr_s = -std::numeric_limits<real_t>::infinity(); *thr_j = TB_NONE; *cnt = 0; }
    tb_wave_sync();

    const unsigned* lst = a.adj_ix + it.p0;
    const real_t* fac = a.adj_f + it.p0;
    const unsigned npass = (it.len + 63) / 64;
    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };   // (tb_gather.hpp) this lane loads piece fq + 4 g of rows frow + 16 r
    ti_u32x4 pre[TI_NI];

    real_t thr = -std::numeric_limits<real_t>::infinity();
    unsigned thj = TB_NONE;
    // lane l owns cell l of the pass: its item and, loaded with it, its factor
    unsigned j_cur = lane < it.len ? lst[lane] : TB_NONE;
    real_t f_cur = lane < it.len ? fac[lane] : (real_t)0;
    unsigned j_nxt = 64 + lane < it.len ? lst[64 + lane] : TB_NONE;
    real_t f_nxt = 64 + lane < it.len ? fac[64 + lane] : (real_t)0;
    if (npass) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);

    for (unsigned pass = 0; pass < npass; pass++) {
        const real_t s = ta_mul(ti_pass(g, pre, As, j_cur, j_nxt, pass, npass), f_cur);
        // ---- selection: the list has room for 64 more ----
        bool appended = false;
        if (j_cur != TB_NONE && s >= thr && (s > thr || j_cur < thj) && !tb_excluded(a.excl, it.ui, arow, j_cur)) {
            const unsigned pos = atomicAdd(cnt, 1u);   // (LDS, integer)
            Ls[pos] = s;
            Li[pos] = j_cur;
            appended = true;
        }
        if (__ballot(appended)) {
            tb_wave_sync();
            const unsigned c = *cnt;
            if (c > a.n_top) {   // (fewer than 64 slots left)
                tb_prune(Ls, Li, c, a.n_top, cnt, thr_s, thr_j);
                thr = *thr_s;
                thj = *thr_j;
            }
        }
        j_cur = j_nxt;
        f_cur = f_nxt;
        const unsigned nx = (pass + 2) * 64 + lane;
        j_nxt = nx < it.len ? lst[nx] : TB_NONE;
        f_nxt = nx < it.len ? fac[nx] : (real_t)0;
    }

    // ---- the slice's answer: the best min(count, n_top) in order, the rest marked empty ----
    tb_wave_sync();
    tb_prune(Ls, Li, *cnt, a.n_top, cnt, thr_s, thr_j);
    const unsigned c = *cnt;
    const size_t o = (size_t)it.dst * a.n_top;
    for (unsigned i = lane; i < a.n_top; i += 64) {
        a.part_score[o + i] = i < c ? Ls[i] : -std::numeric_limits<real_t>::infinity();
        a.part_ix[o + i] = i < c ? Li[i] : TB_NONE;
    }
}

// ---- merge ----
// One wave per user: the best n_top of its dense and sparse lists, which lie side by side in rows first[u] .. first[u + 1] - 1
// (topn_include.hip's ragged merge, with the rows of both stages).
__global__ __launch_bounds__(64) void topn_adjust_merge_kernel(const real_t* part_score, const unsigned* part_ix, const unsigned* first, unsigned n_top,
                                                               real_t* out_score, unsigned* out_ix)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX];
    const unsigned u = blockIdx.x;
    const unsigned ns = first[u + 1] - first[u];
    const size_t o = (size_t)first[u] * n_top;
    real_t* o_score = out_score + (size_t)u * n_top;
    unsigned* o_ix = out_ix + (size_t)u * n_top;
    tb_merge_lists(ms, mj, part_score + o, part_ix + o, ns, n_top, o_score, o_ix);
    tb_merge_pad(mj, ns, n_top, o_score, o_ix);   // a short row: ranks that no real entry reached
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.  The per-user parts and the lists are
// sized from what the budget leaves beside a full exclusion area and the longest adjust row, so that no argument can push it over.
struct TaLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // united exclusion indices a chunk may carry
    size_t adj_cap;          // adjust cells a chunk may carry
    size_t item_cap;         // work items of its sparse stage
    size_t part_rows;        // rows of its partial lists: users x dense slices + the users' sparse slices
    size_t users, ex_indptr, ex_indices, adj_ix, adj_f, items, first, part_score, part_ix, out_score, out_ix, total;
    TaLayout(size_t n_users, size_t n_cells, size_t n_top, size_t dimB)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), TA_MAX_ITEMS);
        const size_t row = n_top * (R + 4);
        adj_cap = std::min(TA_MAX_ROW, std::max<size_t>(n_cells, 1));               // (a row is no longer than the list)
        const size_t rest = TB_BUDGET - TA_IDX_MAX * sizeof(unsigned) - TA_MAX_ROW * TA_CELL - 1024;   // (1024: alignment of the eleven parts)
        // a row of len cells has at most len / TA_SLICE_MIN + 1 work items
        const size_t more_items = adj_cap / TA_SLICE_MIN + 1;
        const size_t per_user = 3 * sizeof(unsigned) + sizeof(TaItem) + row;        // row of A, row pointer, first list row; a work item; the result
        // half of the rest at most for the per-user parts: the lists take what they leave
        size_t uc = std::min({ (rest / 2 - more_items * sizeof(TaItem)) / per_user, TB_CHUNK_USERS_MAX, n_users });
        if (uc > TB_TU) uc -= uc % TB_TU;
        chunk_users = uc;
        idx_cap = std::min(TA_IDX_MAX, uc * dimB);                                  // (no overflow: 2^18 x 2^24)
        item_cap = uc + more_items;
        // users x dense slices <= TB_TU x (TA_TARGET_WGS + tiles)  (tb_slices); the sparse slices the cut charges (ta_slices_bound): at
        // most cells / TA_SLICE_MIN + 1 per row, and no more than the merge allows a user
        const size_t want = std::min(uc * ta_dense_max(n_top), TB_TU * TA_TARGET_WGS + TB_TU + uc) + std::min(uc * ta_sparse_max(n_top), uc + more_items);
        const size_t room = (rest - (uc + 1) * per_user - more_items * sizeof(TaItem)) / row;
        part_rows = std::max(ta_lists_max(n_top), std::min(want, room));            // (room >= one user's lists: it is tens of thousands of rows)
        TbTake take;
        users = take(uc * sizeof(unsigned));
        ex_indptr = take((uc + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        adj_ix = take(adj_cap * sizeof(unsigned));
        adj_f = take(adj_cap * R);
        items = take(item_cap * sizeof(TaItem));
        first = take((uc + 1) * sizeof(unsigned));
        part_score = take(part_rows * n_top * R);
        part_ix = take(part_rows * n_top * sizeof(unsigned));
        out_score = take(uc * n_top * R);
        out_ix = take(uc * n_top * sizeof(unsigned));
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_adjusted_scratch_bytes(size_t n_users, size_t n_cells, size_t n_top, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TaLayout(n_users, n_cells, n_top, dimB).total;
}

extern "C" size_t poismf_hip_topn_adjusted_slices(size_t len, size_t n_top, int bound)
{
    n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
    return bound ? ta_slices_bound(len, n_top) : ta_slices_of(len, n_top);
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_adjusted_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                   const sparse_ix* adj_indptr, const sparse_ix* adj_indices, const real_t* adj_factor,
                                   const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > TA_MAX_ITEMS || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || adj_indptr == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (!tb_rows_ok(adj_indptr, adj_indices, n_users, dimB, TA_MAX_ROW)) return 2;
    const size_t p0 = (size_t)adj_indptr[0], p1 = (size_t)adj_indptr[n_users];
    if (p1 > p0 && adj_factor == nullptr) return 2;
    for (size_t p = p0; p < p1; p++)
        if (!std::isfinite(adj_factor[p]) || adj_factor[p] < (real_t)0) return 2;   // (-0 is 0)
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TA_IDX_MAX)) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_adjusted_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                 const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* adj_indptr,
                                 const sparse_ix* adj_indices, const real_t* adj_factor, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                 const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t n_cells = (size_t)adj_indptr[n_users] - (size_t)adj_indptr[0];
    const TaLayout L(n_users, n_cells, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, 0);
    const size_t lds_dense = tb_lds_bytes(cap, 0);
    if (lds_dense > TB_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the deepest n_top)
    auto dense = topn_adjust_tile_kernel<real_t, sizeof(real_t) == 4, false>;
    auto dense_table = topn_adjust_tile_kernel<real_t, sizeof(real_t) == 4, true>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dense), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dense_table), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));
    const size_t lds_sparse = TA_WAVES * ta_wave_lds(k);
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(topn_adjust_sparse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(TA_WAVES * ta_wave_lds(TB_K_MAX))));

    const TbChunkDev dev = tb_chunk_dev(base, L);
    real_t* const d_out_score = (real_t*)(base + L.out_score);
    unsigned* const d_out_ix = (unsigned*)(base + L.out_ix);
    TaDenseArgs a;
    TaSparseArgs b;
    std::vector<unsigned> hu, hp, hx, hai, hfirst, hix;
    std::vector<sparse_ix> cptr, cidx;   // the chunk's united exclusion rows, from 0
    std::vector<size_t> alen;            // cells a chunk user's adjust row keeps
    std::vector<real_t> haf;
    std::vector<TaItem> items;
    auto row_len = [](const sparse_ix* indptr, size_t i) { return indptr ? (size_t)indptr[i + 1] - (size_t)indptr[i] : 0; };
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose united exclusion rows, adjust cells and partial lists fit their areas together.  The
        // lengths before the rows are united and filtered bound what they come to; a single user always fits
        size_t nu = 0;
        for (size_t cells = 0, idx = 0, ns_sum = 0; u0 + nu < n_users && nu < L.chunk_users; nu++) {
            const size_t len_a = row_len(adj_indptr, u0 + nu), len_e = row_len(excl_indptr, u0 + nu);
            const size_t ns = ta_slices_bound(len_a, n_top);   // (no less than what the row takes once the excluded cells are gone)
            const size_t nd = tb_slices(pmf_ceil_div(nu + 1, TB_TU), dimB, TA_TARGET_WGS, ta_dense_max(n_top)).nslices;
            if (nu > 0 && (cells + len_a > L.adj_cap || idx + len_a + len_e > L.idx_cap || (nu + 1) * nd + ns_sum + ns > L.part_rows)) break;
            cells += len_a;
            idx += len_a + len_e;
            ns_sum += ns;
        }
        // the chunk's rows: the union of the caller's exclusion row and the adjust row's indices for the dense stage, and the adjust
        // row without the cells the caller excludes for the sparse one (both rows are strictly ascending: one pass over the two)
        cptr.assign(1, 0);
        cidx.clear();
        hai.clear();
        haf.clear();
        alen.resize(nu);
        for (size_t i = 0; i < nu; i++) {
            size_t pa = (size_t)adj_indptr[u0 + i], pe = excl_indptr ? (size_t)excl_indptr[u0 + i] : 0;
            const size_t pa1 = (size_t)adj_indptr[u0 + i + 1], pe1 = excl_indptr ? (size_t)excl_indptr[u0 + i + 1] : 0;
            const size_t kept0 = hai.size();
            while (pa < pa1 || pe < pe1) {
                if (pe == pe1 || (pa < pa1 && (size_t)adj_indices[pa] < (size_t)excl_indices[pe])) {
                    cidx.push_back(adj_indices[pa]);
                    hai.push_back((unsigned)adj_indices[pa]);
                    haf.push_back(adj_factor[pa] == (real_t)0 ? (real_t)0 : adj_factor[pa]);   // (-0 is 0)
                    pa++;
                } else {
                    if (pa < pa1 && (size_t)adj_indices[pa] == (size_t)excl_indices[pe]) pa++;   // listed and excluded: excluded
                    cidx.push_back(excl_indices[pe++]);
                }
            }
            cptr.push_back((sparse_ix)cidx.size());
            alen[i] = hai.size() - kept0;
        }
        const size_t nx = cidx.size(), na = hai.size();
        if (nx > L.idx_cap || na > L.adj_cap) return 1;   // (cannot happen: a united row is no longer than dimB, an adjust row than the list)
        hu.resize(nu);
        for (size_t i = 0; i < nu; i++) hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
        TB_TRY(pmf_upload(dev.users, hu.data(), nu * sizeof(unsigned), stream));
        TB_TRY(tb_stage_excl(a.excl, seen, nx ? cptr.data() : nullptr, cidx.data(), 0, nu, nx, dev.ex_indptr, dev.ex_indices, hp, hx, stream));

        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, TA_TARGET_WGS, ta_dense_max(n_top));   // (the merge kernel's LDS bounds them)
        const size_t nd = sl.nslices;
        // the plan of the sparse stage: one work item per (user, slice of its adjust row), its list behind the user's dense ones
        hfirst.resize(nu + 1);
        hfirst[0] = 0;
        for (size_t i = 0; i < nu; i++) hfirst[i + 1] = hfirst[i] + (unsigned)(nd + ta_slices_of(alen[i], n_top));
        if (hfirst[nu] > L.part_rows) return 1;    // (cannot happen: the chunk was cut with ta_slices_bound of the rows before they lost cells)
        const bool direct = na == 0 && nd == 1;    // section 1f with one slice: its sorted, padded lists are the results
        a.A = dA;
        a.B = dB;
        a.users = dev.users;
        a.n_users = (unsigned)nu;
        a.dimB = (unsigned)dimB;
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.cap = (unsigned)cap;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        a.nslices = (unsigned)nd;
        a.first = na > 0 ? (const unsigned*)(base + L.first) : nullptr;
        a.part_score = direct ? d_out_score : (real_t*)(base + L.part_score);
        a.part_ix = direct ? d_out_ix : (unsigned*)(base + L.part_ix);
        if (na > 0) TB_TRY(pmf_upload(base + L.first, hfirst.data(), (nu + 1) * sizeof(unsigned), stream));
        hipLaunchKernelGGL(na > 0 ? dense_table : dense, dim3((unsigned)tiles, (unsigned)nd), dim3(TB_WG), lds_dense, stream, a);
        TB_TRY(hipGetLastError());
        if (na > 0) {
            items.clear();
            for (size_t i = 0, p0 = 0; i < nu; p0 += alen[i], i++) {
                const size_t len = alen[i], ns = ta_slices_of(len, n_top), slice = ta_slice(len, n_top);
                for (size_t s = 0; s < ns; s++)
                    items.push_back({ (unsigned)i, (unsigned)(p0 + s * slice), (unsigned)std::min(slice, len - s * slice), (unsigned)(hfirst[i] + nd + s) });
            }
            if (items.size() > L.item_cap) return 1;   // (cannot happen: a row of len cells has at most len / TA_SLICE_MIN + 1 work items)
            TB_TRY(pmf_upload(base + L.adj_ix, hai.data(), na * sizeof(unsigned), stream));
            TB_TRY(pmf_upload(base + L.adj_f, haf.data(), na * sizeof(real_t), stream));
            TB_TRY(pmf_upload(base + L.items, items.data(), items.size() * sizeof(TaItem), stream));
            b.A = dA;
            b.B = dB;
            b.users = dev.users;
            b.items = (const TaItem*)(base + L.items);
            b.n_items = (unsigned)items.size();
            b.adj_ix = (const unsigned*)(base + L.adj_ix);
            b.adj_f = (const real_t*)(base + L.adj_f);
            b.k = (int)k;
            b.n_top = (unsigned)n_top;
            b.excl = a.excl;
            b.excl.ex_indptr = nullptr;   // (the caller's cells are gone from the adjust rows already)
            b.part_score = a.part_score;
            b.part_ix = a.part_ix;
            hipLaunchKernelGGL(topn_adjust_sparse_kernel, dim3((unsigned)pmf_ceil_div(items.size(), TA_WAVES)), dim3(64 * TA_WAVES), lds_sparse, stream, b);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(topn_adjust_merge_kernel, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, a.first, (unsigned)n_top,
                               d_out_score, d_out_ix);
            TB_TRY(hipGetLastError());
        } else if (nd > 1) {
            hipLaunchKernelGGL(topn_merge_kernel<true>, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, (unsigned)nu, (unsigned)nd,
                               (unsigned)n_top, d_out_score, d_out_ix);
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, d_out_ix, d_out_score, hix, out_ix, out_score, stream)) return 1;
        u0 += nu;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_adjusted(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                             size_t n_top, const sparse_ix* adj_indptr, const sparse_ix* adj_indices, const real_t* adj_factor,
                             const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_adjusted_check(users, n_users, n_top, dimA, dimB, (size_t)k, adj_indptr, adj_indices, adj_factor, excl_indptr,
                                                      excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_adjusted_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, adj_indptr, adj_indices,
                                                             adj_factor, nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
