// rank_shared.hip -- batched exact ranks among candidate lists shared between users (include/poismf_hip.h, section 1k): a table of lists,
// every user refers to one of them, and each held-out item of a user gets its 0-based position among C(u) = L_{list_of(u)} \ E(u) --
// with unite_test, (L_{list_of(u)} united with T(u)) \ E(u) -- under the total order "score descending, item index ascending".
// score(u, j) is section 1f's: the k-ordered fused chain, bit for bit what pair_dot_kernel (serve.hip) computes.
//
// rank(u, t) = #{j in L before t} - #{e in E(u) and in L before t} + #{t' in T(u) \ L, not in E(u), before t}  (the last: united mode)
//
//   rank_shared_threshold_kernel  one thread per held-out cell: its score with the scalar chain (the "threshold"), whether it is in
//                          E(u), and whether it is listed (a binary search in the user's list inside the resident table).  Valid: not
//                          in E(u), and (listed or unite_test).
//   rank_order_kernel      (tb_rank.hpp, unchanged) valid thresholds best first under the total order, the others behind them.
//   rank_shared_kernel     rank_tile_kernel's counting epilogue (rank_batch.hip) on topn_shared_kernel's gathered item tile
//                          (topn_shared.hip).  A row of the tile is a GROUP: up to RS_G consecutive ordered thresholds of one user.  The
//                          host puts a chunk's users in order of their list (a stable counting sort) and packs their groups into tiles
//                          of at most TB_TU = 64 groups that refer to the same list; a workgroup owns one tile and one slice of its
//                          list, which it walks TB_TJ = 64 candidates at a time through tb_walk -- tile row r of the step at list
//                          position p is row lst[p + r] of B, "no row" (zeros) past the list's end -- so a row of B read once serves 64
//                          groups.  Counting is rank_tile_kernel's: best and worst threshold in registers, the thresholds between them
//                          from LDS, integer LDS bins.  A candidate is admitted by its POSITION in the list (p < len), never by its
//                          score: an all-zero row of A scores 0 against a phantom zero row too.  Ties are broken by the candidate's
//                          item index from the list (fetched one step ahead, like the rows it names).  Slices add their running sums
//                          to the global counters with integer atomics (order cannot matter); a (tile, slice) that starts past its
//                          list's end leaves at once.  The tile's score of a listed t has the bits of t's threshold, so t never comes
//                          before itself.
//   rank_shared_excl_kernel  one wave per chunk user over E(u) (the batch's list, then the resident row minus what the list already
//                          had): an excluded item that is in the user's list gets the scalar score, a binary search in the user's
//                          ordered thresholds and +1 in a difference array at the first threshold it comes before; listed items
//                          n_listed = |L| - |E(u) and L|.
//   rank_shared_finish_kernel  one thread per user: rank = dense count - running sum of the difference array + the valid unlisted
//                          thresholds ordered before this one (by the total order exactly the members of T(u) \ L before it);
//                          N(u) = n_listed + the valid unlisted thresholds.  A user without a valid threshold has no tile row and
//                          still gets N(u).
//
// All counting is in integers; no float atomics.  The host side touches `users`, `list_of`, the table, the held-out and the exclusion
// lists only: nothing is proportional to users x list length.  The table goes up once per call, narrowed to 32 bits; ONE scratch
// allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds it and a chunk's parts (RsLayout; poismf_hip_rank_shared_scratch_bytes
// reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <new>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_rank.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int RS_G = 32;                                  // thresholds per row of the tile
constexpr int RS_GS = RS_G + 1;                           // LDS row stride of thresholds and bins (rows 4 apart fall on banks 4 apart)
constexpr size_t RS_TARGET_WGS = 768;                     // lists are split over workgroups until a chunk has about this many
constexpr size_t RS_MAX_CELLS = POISMF_HIP_TOPN_SHARED_MAX_CELLS;
constexpr size_t RS_CHUNK_CELLS = POISMF_HIP_RANK_SHARED_CHUNK_CELLS;
static_assert(RS_MAX_CELLS * sizeof(unsigned) == TB_BUDGET / 4, "the list table fills a quarter of the scratch at most");

struct RsTile { unsigned l0, len, first, count; };        // the list (start in the table's index area, length), first group, groups <= TB_TU

struct RsArgs {
    RbArgs r;                         // (tb_rank.hpp) grow / gstart: the chunk's groups in order of their list
    const unsigned* lists;            // the table's indices, one row after the other
    const unsigned* ul0;              // [n_users] where the chunk user's list starts in `lists` ...
    const unsigned* ulen;             // ... and its length
    unsigned* cell_unl;               // [n_cells] 1: a valid cell whose item is not in the user's list (united mode only)
    const RsTile* tiles;
    int unite;
};

__global__ __launch_bounds__(256) void rank_shared_threshold_kernel(RsArgs a)
{
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.r.n_cells) return;
    const unsigned i = a.r.cell_row[c], j = a.r.cell_item[c];
    a.r.cell_score[c] = rb_dot(a.r.A, a.r.B, a.r.k, a.r.arow[i], j);
    const unsigned l0 = a.ul0[i];
    const bool listed = tb_sorted_has(a.lists, l0, (unsigned long long)l0 + a.ulen[i], j);
    const bool out = tb_excluded(a.r.excl, i, a.r.arow[i], j) || !(listed || a.unite != 0);
    a.r.cell_excl[c] = out ? 1u : 0u;
    a.cell_unl[c] = !out && !listed ? 1u : 0u;
}

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void rank_shared_kernel(RsArgs a)
{
    extern __shared__ __align__(16) unsigned char rs_smem[];
    T* As = (T*)rs_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    T* Ts = Bs + TB_TJ * TB_KS;                           // [TB_TU][RS_GS] a group's thresholds, best first: score ...
    unsigned* Tj = (unsigned*)(Ts + TB_TU * RS_GS);       // ... and item
    unsigned* bins = Tj + TB_TU * RS_GS;                  // [TB_TU][RS_GS] candidates whose first beaten threshold is this one
    unsigned* uid = bins + TB_TU * RS_GS;                 // [TB_TU] row of A, TB_NONE for a row without thresholds
    unsigned* gn = uid + TB_TU;                           // [TB_TU] thresholds in the group
    unsigned* gs = gn + TB_TU;                            // [TB_TU] its first ordered entry

    const RsTile tile = a.tiles[blockIdx.x];
    const unsigned len = tile.len;
    const unsigned ntiles = (len + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.r.tiles_per_slice;
    if (tile0 >= ntiles) return;                          // (the whole workgroup, before any barrier) this slice starts past the list's end
    const unsigned tile1 = tile0 + a.r.tiles_per_slice < ntiles ? tile0 + a.r.tiles_per_slice : ntiles;
    const unsigned* lst = a.lists + tile.l0;

    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TB_TU) {
        unsigned u = TB_NONE, n = 0, st = 0;
        if (tid < tile.count) {
            const unsigned g = tile.first + tid;
            const unsigned row = a.r.grow[g];
            st = a.r.gstart[g];
            const unsigned off = st - a.r.tptr[row], nv = a.r.nvalid[row];
            if (nv > off) n = nv - off < (unsigned)RS_G ? nv - off : (unsigned)RS_G;
            if (n > 0) u = a.r.arow[row];
        }
        uid[tid] = u;
        gn[tid] = n;
        gs[tid] = st;
    }
    __syncthreads();
    for (unsigned e = tid; e < (unsigned)(TB_TU * RS_G); e += TB_WG) {
        const unsigned row = e / RS_G, i = e % RS_G;
        const bool in = i < gn[row];
        Ts[row * RS_GS + i] = in ? a.r.s_score[gs[row] + i] : (T)0;
        Tj[row * RS_GS + i] = in ? a.r.s_item[gs[row] + i] : 0u;
        bins[row * RS_GS + i] = 0;
    }
    __syncthreads();

    const unsigned col = lane & 15, quad = lane >> 4;
    const unsigned urow0 = 16 * wave + 4 * quad;          // this lane's four rows are urow0 .. urow0 + 3
    auto user_row = [&](int row) { const unsigned r = uid[row]; return r == TB_NONE ? -1ll : (long long)r; };
    // tile row `row` of the step at list position p: the list's entry there, none past its end
    auto item_rows = [lst, len](unsigned p) {
        return [lst, len, p](int row) { const unsigned q = p + (unsigned)row; return q < len ? (long long)lst[q] : -1ll; };
    };

    // best and worst threshold of this lane's four rows; a row without thresholds has a worst one nothing comes before
    T best_s[4], worst_s[4];
    unsigned best_j[4], worst_j[4], n_r[4], all_r[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const unsigned n = gn[urow0 + r];
        n_r[r] = n;
        all_r[r] = 0;
        best_s[r] = Ts[(urow0 + r) * RS_GS];
        best_j[r] = Tj[(urow0 + r) * RS_GS];
        worst_s[r] = n > 0 ? Ts[(urow0 + r) * RS_GS + n - 1] : std::numeric_limits<T>::infinity();
        worst_j[r] = n > 0 ? Tj[(urow0 + r) * RS_GS + n - 1] : 0u;
    }

    // this lane's four candidates of a step, fetched one step ahead like the rows they name
    unsigned j_next[4];
    auto fetch_items = [&](unsigned p) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned q = p + 16 * t + col;
            j_next[t] = q < len ? lst[q] : TB_NONE;
        }
    };
    fetch_items(tile0 * TB_TJ);

    tb_walk<T, MFMA>(As, Bs, a.r.A, a.r.B, a.r.k, tile0, tile1, user_row, item_rows, [&](T (&acc)[4][4], unsigned p_base) {
        unsigned j_cur[4];
#pragma unroll
        for (int t = 0; t < 4; t++) j_cur[t] = j_next[t];
        if (p_base + TB_TJ < tile1 * TB_TJ) fetch_items(p_base + TB_TJ);
        // ---- counting: the bins of rows 16 wave .. 16 wave + 15 are touched by this wave alone ----
#pragma unroll
        for (int r = 0; r < 4; r++) {
            bool some[4], any = false;   // comes before some threshold: before the worst one
#pragma unroll
            for (int t = 0; t < 4; t++) {
                // (by position: a phantom row past the list's end scores 0 like any zero row)
                some[t] = p_base + 16 * t + col < len && tb_better(acc[t][r], j_cur[t], worst_s[r], worst_j[r]);
                any = any || some[t];
            }
            if (__ballot(any) == 0) continue;       // (uniform over the wave) every score of this pass died in registers
            bool mid[4], any_mid = false;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool all = some[t] && tb_better(acc[t][r], j_cur[t], best_s[r], best_j[r]);   // before all of them
                all_r[r] += all ? 1u : 0u;
                mid[t] = some[t] && !all;
                any_mid = any_mid || mid[t];
            }
            if (__ballot(any_mid) == 0) continue;   // (uniform) the survivors counted in registers
            // before the worst threshold, not before the best: how many of thresholds 1 .. n - 2 it comes before besides.  The row's
            // thresholds are read once for the lane's four scores (the same address for the 16 lanes of a row: a broadcast); the
            // item indices are only looked at when some lane of the wave meets an equal score.
            const T* ts = Ts + (urow0 + r) * RS_GS;
            const unsigned* tj = Tj + (urow0 + r) * RS_GS;
            const unsigned n = n_r[r];
            unsigned beaten[4] = { 1, 1, 1, 1 };
            for (unsigned i = 1; i + 1 < n; i++) {
                const T ti = ts[i];
#pragma unroll
                for (int t = 0; t < 4; t++) beaten[t] += acc[t][r] > ti ? 1u : 0u;
                const bool tie = acc[0][r] == ti || acc[1][r] == ti || acc[2][r] == ti || acc[3][r] == ti;
                if (__ballot(tie) != 0) {
                    const unsigned ji = tj[i];
#pragma unroll
                    for (int t = 0; t < 4; t++) beaten[t] += acc[t][r] == ti && j_cur[t] < ji ? 1u : 0u;
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (mid[t]) atomicAdd(&bins[(urow0 + r) * RS_GS + n - beaten[t]], 1u);   // (LDS, integer) the first threshold it comes before
        }
    });

    // ---- the slice's counts: a candidate before the best threshold is before every one of the group ----
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (all_r[r]) atomicAdd(&bins[(urow0 + r) * RS_GS], all_r[r]);
    __syncthreads();
    if (tid < TB_TU) {
        const unsigned n = gn[tid];
        unsigned run = 0;
        for (unsigned i = 0; i < n; i++) {
            run += bins[tid * RS_GS + i];
            if (run) atomicAdd(&a.r.dense[gs[tid] + i], run);   // (global, integer: the slices' counts add up in any order)
        }
    }
}

// one wave per chunk user
__global__ __launch_bounds__(256) void rank_shared_excl_kernel(RsArgs a)
{
    const unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.r.n_users) return;   // (uniform over the wave)
    const unsigned p0 = a.r.tptr[i], nv = a.r.nvalid[i], u = a.r.arow[i];
    const unsigned long long l0 = a.ul0[i], l1 = l0 + a.ulen[i];
    const real_t* ts = a.r.s_score + p0;
    const unsigned* tj = a.r.s_item + p0;
    unsigned n_hit = 0;             // (uniform) members of E(u) that are in the list
    // called by the whole wave: lane's item j of E(u), when `mine`, leaves the counts it entered as a member of the list
    auto subtract = [&](bool mine, unsigned j) {
        const bool hit = mine && tb_sorted_has(a.lists, l0, l1, j);
        if (hit && nv > 0) {
            const unsigned pos = rb_first_beaten(ts, tj, nv, rb_dot(a.r.A, a.r.B, a.r.k, u, j), j);
            if (pos < nv) atomicAdd(&a.r.corr[p0 + pos], 1u);
        }
        n_hit += (unsigned)__popcll(__ballot(hit));
    };
    unsigned long long e0 = 0, e1 = 0;
    const TbExcl& x = a.r.excl;
    if (x.ex_indptr != nullptr) {
        e0 = x.ex_indptr[i];
        e1 = x.ex_indptr[i + 1];
        for (unsigned long long base = e0; base < e1; base += 64) {
            const unsigned long long p = base + lane;
            subtract(p < e1, p < e1 ? x.ex_indices[p] : 0u);
        }
    }
    if (x.seen_indptr != nullptr) {
        const unsigned row = u - x.seen_row0;
        const unsigned long long s0 = x.seen_indptr[row], s1 = x.seen_indptr[row + 1];
        for (unsigned long long base = s0; base < s1; base += 64) {
            const unsigned long long p = base + lane;
            bool mine = p < s1;
            unsigned j = 0;
            if (mine) {
                j = x.seen_indices[p];
                if (x.ex_indptr != nullptr && tb_sorted_has(x.ex_indices, e0, e1, j)) mine = false;   // the list had it
                if (mine && !x.seen_sorted)   // a row in the caller's own order may name an item twice: the first one counts
                    for (unsigned long long q = s0; q < p && mine; q++) mine = x.seen_indices[q] != j;
            }
            subtract(mine, j);
        }
    }
    if (lane == 0) a.r.n_adm[i] = a.ulen[i] - n_hit;
}

// one thread per chunk user, after rank_shared_excl_kernel
__global__ __launch_bounds__(256) void rank_shared_finish_kernel(RsArgs a)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.r.n_users) return;
    const unsigned p0 = a.r.tptr[i], p1 = a.r.tptr[i + 1], nv = a.r.nvalid[i];
    unsigned run = 0, unl = 0;   // excluded members of the list, valid unlisted thresholds: those ordered before the entry at hand
    for (unsigned p = p0; p < p1; p++) {
        const unsigned o = a.r.s_origin[p];
        if (p - p0 < nv) {
            run += a.r.corr[p];
            a.r.rank[o] = a.r.dense[p] - run + unl;
            unl += a.cell_unl[o];
        } else
            a.r.rank[o] = RB_EXCLUDED;
    }
    if (unl) a.r.n_adm[i] += unl;
}

// The one scratch allocation of a call: the list table and what a chunk of users needs, in bytes from the start.  Every capacity grows
// (or stays) when an argument grows, and none depends on another's, so the total never decreases.
constexpr size_t RS_PARTS = 23;
constexpr size_t RS_PER_USER = 7 * sizeof(unsigned) + 2 * sizeof(unsigned) + sizeof(RsTile);   // seven per-user arrays, a group and a tile of its own
constexpr size_t RS_PER_CELL = 9 * sizeof(unsigned) + 2 * sizeof(real_t);                      // nine index arrays, two of scores
constexpr size_t RS_PER_GROUP = 2 * sizeof(unsigned) + sizeof(RsTile);
struct RsLayout {
    size_t chunk_users;      // users per chunk
    size_t list_cap;         // indices of the list table
    size_t cell_cap;         // held-out cells a chunk may carry
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t group_cap;        // groups (and, at worst, tiles) of a chunk
    size_t lists, arow, tptr, ex_indptr, nvalid, n_adm, ul0, ulen, cell_row, cell_item, cell_score, cell_excl, cell_unl, s_score, s_item,
        s_origin, dense, corr, rank, grow, gstart, tiles, ex_indices, total;
    RsLayout(size_t n_users, size_t n_test, size_t n_list_cells, size_t dimB)
    {
        const size_t R = sizeof(real_t), U = sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        dimB = std::max<size_t>(dimB, 1);
        chunk_users = std::min(n_users, TB_CHUNK_USERS_MAX);
        list_cap = std::min(RS_MAX_CELLS, std::max<size_t>(n_list_cells, 1));             // a quarter of the budget at most
        idx_cap = std::min(TB_BUDGET / 2 / U, chunk_users * dimB);                         // section 1f's: half of it  (no overflow: 2^18 x 2^31)
        cell_cap = std::min(RS_CHUNK_CELLS, std::max<size_t>(n_test, 1));                  // (with the users' parts a quarter at most: see below)
        group_cap = chunk_users + cell_cap / RS_G + 1;                                     // a user adds at most one partial group
        TbTake take;
        lists = take(list_cap * U);
        arow = take(chunk_users * U);
        tptr = take((chunk_users + 1) * U);
        ex_indptr = take((chunk_users + 1) * U);
        nvalid = take(chunk_users * U);
        n_adm = take(chunk_users * U);
        ul0 = take(chunk_users * U);
        ulen = take(chunk_users * U);
        cell_row = take(cell_cap * U);
        cell_item = take(cell_cap * U);
        cell_score = take(cell_cap * R);
        cell_excl = take(cell_cap * U);
        cell_unl = take(cell_cap * U);
        s_score = take(cell_cap * R);
        s_item = take(cell_cap * U);
        s_origin = take(cell_cap * U);
        dense = take(cell_cap * U);
        corr = take(cell_cap * U);
        rank = take(cell_cap * U);
        grow = take(group_cap * U);
        gstart = take(group_cap * U);
        tiles = take(group_cap * sizeof(RsTile));
        ex_indices = take(idx_cap * U);
        total = take.o;
    }
};
// a chunk's cells, users, groups and tiles at their largest, with the alignment of every part, fit the quarter of the budget that the
// table and the exclusion indices leave; and the longest held-out row a call accepts fits a chunk whatever the other arguments are
static_assert(32 * RS_PARTS + 2 * sizeof(unsigned) + RS_PER_GROUP + RS_PER_USER * TB_CHUNK_USERS_MAX + RS_PER_CELL * RS_CHUNK_CELLS +
                      RS_PER_GROUP * (RS_CHUNK_CELLS / RS_G) <= TB_BUDGET / 4,
              "a chunk fits the scratch budget");
static_assert(RS_CHUNK_CELLS >= RB_ROW_MAX, "one held-out row fits a chunk");

size_t rs_lds_bytes() { return 2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + (size_t)TB_TU * RS_GS * (sizeof(real_t) + 8) + (size_t)TB_TU * 12; }
// two workgroups per CU (160 KB of LDS), as rank_tile_kernel
static_assert(2 * (2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + (size_t)TB_TU * RS_GS * (sizeof(real_t) + 8) + (size_t)TB_TU * 12) <= 160 * 1024,
              "two workgroups of rank_shared_kernel per CU");

}  // namespace

extern "C" size_t poismf_hip_rank_shared_scratch_bytes(size_t n_users, size_t n_test_cells, size_t n_lists, size_t n_list_cells, size_t dimB,
                                                       size_t k)
{
    (void)n_lists;   // (a user carries its list's place in the table: no row pointers go to the device)
    (void)k;         // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return RsLayout(n_users, n_test_cells, n_list_cells, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_rank_shared_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                 const sparse_ix* test_indices, const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists,
                                 const sparse_ix* list_of, const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || test_indptr == nullptr || list_indptr == nullptr || list_of == nullptr || n_lists == 0) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA || (size_t)list_of[i] >= n_lists) return 2;
    if ((size_t)list_indptr[n_lists] - (size_t)list_indptr[0] > RS_MAX_CELLS) return 2;   // (the table as a whole, before an index is read)
    if (!tb_rows_ok(list_indptr, list_indices, n_lists, dimB, RS_MAX_CELLS)) return 2;
    if (!tb_rows_ok(test_indptr, test_indices, n_users, dimB, RB_ROW_MAX)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_rank_shared_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                               const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                               const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of,
                               bool unite_test, PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                               void** d_scratch, size_t* scratch_cap, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t n_test = (size_t)test_indptr[n_users] - (size_t)test_indptr[0];
    const size_t l_base = (size_t)list_indptr[0];
    const size_t n_list_cells = (size_t)list_indptr[n_lists] - l_base;
    const RsLayout L(n_users, n_test, n_list_cells, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;
    const size_t lds = rs_lds_bytes();
    auto kern = rank_shared_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    RsArgs a;
    RbArgs& r = a.r;
    std::vector<unsigned> hl, hu, htp, hl0, hlen, hrow, hitem, hperm, hgrow, hgstart, hp, hx, touched, count;
    std::vector<RsTile> tiles;
    try {
        // the table: once per call, narrowed to 32 bits
        hl.resize(n_list_cells);
        for (size_t p = 0; p < n_list_cells; p++) hl[p] = (unsigned)list_indices[l_base + p];
        count.assign(n_lists, 0u);   // users of each list in the chunk at hand; all zero between chunks
    } catch (const std::bad_alloc&) { return 1; }
    TB_TRY(pmf_upload(base + L.lists, hl.data(), n_list_cells * sizeof(unsigned), stream));
    auto row_len = [](const sparse_ix* indptr, size_t i) { return indptr ? (size_t)indptr[i + 1] - (size_t)indptr[i] : 0; };

    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users consecutive users whose held-out cells and exclusion lists fit their areas together
        size_t u1 = u0, nc = 0, nx = 0;
        while (u1 < n_users && u1 - u0 < L.chunk_users) {
            const size_t cells = row_len(test_indptr, u1), len_e = row_len(excl_indptr, u1);
            if (u1 > u0 && (nc + cells > L.cell_cap || nx + len_e > L.idx_cap)) break;
            nc += cells;
            nx += len_e;
            u1++;
        }
        const size_t nu = u1 - u0;
        if (nc > L.cell_cap || nx > L.idx_cap) return 1;   // (cannot happen: the checks bound a single row by both)
        const size_t c_base = (size_t)test_indptr[u0];
        hu.resize(nu);
        htp.resize(nu + 1);
        hl0.resize(nu);
        hlen.resize(nu);
        hrow.resize(nc);
        hitem.resize(nc);
        touched.clear();
        for (size_t i = 0; i < nu; i++) {
            hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
            const size_t p0 = (size_t)test_indptr[u0 + i] - c_base, p1 = (size_t)test_indptr[u0 + i + 1] - c_base;
            htp[i] = (unsigned)p0;
            for (size_t p = p0; p < p1; p++) {
                hrow[p] = (unsigned)i;
                hitem[p] = (unsigned)test_indices[c_base + p];
            }
            const size_t g = (size_t)list_of[u0 + i];
            hl0[i] = (unsigned)((size_t)list_indptr[g] - l_base);
            hlen[i] = (unsigned)row_len(list_indptr, g);
            if (count[g]++ == 0) touched.push_back((unsigned)g);
        }
        htp[nu] = (unsigned)nc;

        // the users in order of their list (a stable counting sort over the lists the chunk refers to); their groups of RS_G cells in
        // that order, cut into tiles of one list each.  An empty list has no tile: nothing is counted against its users' thresholds.
        std::sort(touched.begin(), touched.end());
        size_t first = 0;
        for (const unsigned g : touched) {
            const size_t c = count[g];
            count[g] = (unsigned)first;   // (from here on: where the list's next user goes)
            first += c;
        }
        hperm.resize(nu);
        for (size_t i = 0; i < nu; i++) hperm[count[(size_t)list_of[u0 + i]]++] = (unsigned)i;
        for (const unsigned g : touched) count[g] = 0;
        hgrow.clear();
        hgstart.clear();
        tiles.clear();
        size_t max_len = 0;
        for (size_t s = 0, g_first = 0; s < nu; s++) {
            const unsigned i = hperm[s];
            for (size_t p = htp[i]; p < htp[i + 1]; p += RS_G) {
                hgrow.push_back(i);
                hgstart.push_back((unsigned)p);
            }
            if (s + 1 < nu && list_of[u0 + hperm[s + 1]] == list_of[u0 + i]) continue;
            // the last user of its list: the list's groups are g_first .. hgrow.size() - 1
            const size_t g_end = hgrow.size(), len = hlen[i];
            for (size_t f = g_first; len > 0 && f < g_end; f += TB_TU)
                tiles.push_back({ hl0[i], (unsigned)len, (unsigned)f, (unsigned)std::min<size_t>(TB_TU, g_end - f) });
            if (g_end > g_first) max_len = std::max(max_len, len);
            g_first = g_end;
        }
        const size_t ng = hgrow.size();
        if (ng > L.group_cap || tiles.size() > L.group_cap) return 1;   // (cannot happen: a user adds at most one partial group, a tile holds a group)
        TB_TRY(pmf_upload(base + L.arow, hu.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.tptr, htp.data(), (nu + 1) * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.ul0, hl0.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.ulen, hlen.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_row, hrow.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_item, hitem.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.grow, hgrow.data(), ng * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.gstart, hgstart.data(), ng * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.tiles, tiles.data(), tiles.size() * sizeof(RsTile), stream));
        TB_TRY(tb_stage_excl(r.excl, seen, excl_indptr, excl_indices, u0, nu, nx, (unsigned*)(base + L.ex_indptr), (unsigned*)(base + L.ex_indices), hp,
                             hx, stream));
        TB_TRY(hipMemsetAsync(base + L.nvalid, 0, nu * sizeof(unsigned), stream));
        if (nc > 0) {
            TB_TRY(hipMemsetAsync(base + L.dense, 0, nc * sizeof(unsigned), stream));
            TB_TRY(hipMemsetAsync(base + L.corr, 0, nc * sizeof(unsigned), stream));
        }

        const TbSlices sl = tb_slices(std::max<size_t>(tiles.size(), 1), std::max<size_t>(max_len, 1), RS_TARGET_WGS);
        r.A = dA;
        r.B = dB;
        r.k = (int)k;
        r.dimB = (unsigned)dimB;
        r.n_users = (unsigned)nu;
        r.n_cells = (unsigned)nc;
        r.arow = (const unsigned*)(base + L.arow);
        r.tptr = (const unsigned*)(base + L.tptr);
        r.cell_row = (const unsigned*)(base + L.cell_row);
        r.cell_item = (const unsigned*)(base + L.cell_item);
        r.cell_score = (real_t*)(base + L.cell_score);
        r.cell_excl = (unsigned*)(base + L.cell_excl);
        r.s_score = (real_t*)(base + L.s_score);
        r.s_item = (unsigned*)(base + L.s_item);
        r.s_origin = (unsigned*)(base + L.s_origin);
        r.nvalid = (unsigned*)(base + L.nvalid);
        r.dense = (unsigned*)(base + L.dense);
        r.corr = (unsigned*)(base + L.corr);
        r.rank = (unsigned*)(base + L.rank);
        r.n_adm = (unsigned*)(base + L.n_adm);
        r.grow = (const unsigned*)(base + L.grow);
        r.gstart = (const unsigned*)(base + L.gstart);
        r.ngroups = (unsigned)ng;
        r.nslices = (unsigned)sl.nslices;
        r.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        r.iptr = nullptr;
        r.incl = nullptr;
        a.lists = (const unsigned*)(base + L.lists);
        a.ul0 = (const unsigned*)(base + L.ul0);
        a.ulen = (const unsigned*)(base + L.ulen);
        a.cell_unl = (unsigned*)(base + L.cell_unl);
        a.tiles = (const RsTile*)(base + L.tiles);
        a.unite = unite_test ? 1 : 0;
        if (nc > 0) {
            const unsigned cell_blocks = (unsigned)pmf_ceil_div(nc, 256);
            hipLaunchKernelGGL(rank_shared_threshold_kernel, dim3(cell_blocks), dim3(256), 0, stream, a);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(rank_order_kernel, dim3(cell_blocks), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
            if (!tiles.empty()) {
                hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size(), (unsigned)sl.nslices), dim3(TB_WG), lds, stream, a);
                TB_TRY(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(rank_shared_excl_kernel, dim3((unsigned)pmf_ceil_div(nu, 4)), dim3(256), 0, stream, a);
        TB_TRY(hipGetLastError());
        if (nc > 0) {
            hipLaunchKernelGGL(rank_shared_finish_kernel, dim3((unsigned)pmf_ceil_div(nu, 256)), dim3(256), 0, stream, a);
            TB_TRY(hipGetLastError());
            TB_TRY(pmf_download(out_rank + c_base, base + L.rank, nc * sizeof(unsigned), stream));
        }
        TB_TRY(pmf_download(out_n_adm + u0, base + L.n_adm, nu * sizeof(unsigned), stream));
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_rank_shared(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                           const sparse_ix* test_indptr, const sparse_ix* test_indices, const sparse_ix* list_indptr,
                           const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of, int unite_test,
                           const sparse_ix* excl_indptr, const sparse_ix* excl_indices, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_shared_check(users, n_users, dimA, dimB, (size_t)k, test_indptr, test_indices, list_indptr, list_indices,
                                                    n_lists, list_of, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_rank_shared_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, test_indptr, test_indices,
                                                           list_indptr, list_indices, n_lists, list_of, unite_test != 0, nullptr, excl_indptr,
                                                           excl_indices, d_scratch, scratch_cap, out_rank, out_n_adm);
                     });
}

}  // extern "C"
