// topn_shared.hip -- batched top-N over candidate lists shared between users (include/poismf_hip.h, section 1i): a table of lists, every
// user refers to one of them, and the answer of a user is the n_top best of ITS LIST minus its exclusion set under the total order
// "score descending, item index ascending".
//
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t
//
// bit for bit what pair_dot_kernel (serve.hip), topn_tile_kernel (topn_batch.hip) and topn_include_kernel (topn_include.hip) compute.
//
// The host puts a chunk's users in order of their list (a stable counting sort) and cuts every group into USER TILES of at most
// TB_TU = 64 users that refer to the same list.  topn_shared_kernel is topn_tile_kernel with the item tile gathered by the list: a
// workgroup of four waves owns one user tile and one slice of its list, which it walks TB_TJ = 64 candidates at a time -- tile row r of
// the step at list position p is row lst[p + r] of B, "no row" (zeros) past the list's end -- through tb_walk / tb_compute
// (tb_tile.hpp), so a row of B read once serves 64 users (fp32: v_mfma_f32_16x16x4_f32; fp64: the VALU chain).  A candidate past the
// end of the list is left out by its POSITION, never by its score: an all-zero row of A scores 0 against a phantom zero row too.  The
// selection is tb_select.hpp's (TbSelect, as in topn_batch.hip): a threshold per user held in registers between prunes, tb_excluded, an
// LDS integer counter, tb_prune by rank counting.  No float atomics.  Every tile row carries its user's position in the chunk (the caller's order), which is
// the row of the result, the row of the partial lists and the index tb_excluded wants: results come down already in order.
// A chunk with few user tiles cuts the lists into slices (one slice length per launch, taken from the longest list of the chunk; a
// (tile, slice) that starts past its list's end leaves at once); topn_shared_merge_kernel ranks a user's partial lists
// (tb_merge_lists) and pads what no real entry reaches.  With one slice the tile kernel writes the result rows itself.
//
// The host side touches `users`, `list_of`, the table and the exclusion lists only: nothing is proportional to the sum over users of
// their lists' lengths.  The table goes up once per call, narrowed to 32 bits; ONE scratch allocation of at most
// POISMF_HIP_TOPN_BATCH_BUDGET_MB holds it and a chunk's users, tiles, exclusion lists, partial lists and results (TsLayout;
// poismf_hip_topn_shared_scratch_bytes reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <new>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"

namespace {

constexpr size_t TS_UPOS_BYTES = TB_TU * sizeof(unsigned);   // the tile rows' positions in the chunk, behind the selection in LDS
constexpr size_t TS_TARGET_WGS = 768;                     // lists are split over workgroups until a chunk has about this many
constexpr size_t TS_MAX_CELLS = POISMF_HIP_TOPN_SHARED_MAX_CELLS;
constexpr size_t TS_PART_BYTES = (size_t)32 << 20;        // most a chunk's partial lists take
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, TS_UPOS_BYTES) <= TB_LDS_LIMIT, "the two tiles, 64 lists of the deepest n_top with TB_ROOM free slots and the positions fit LDS");
static_assert(TS_MAX_CELLS * sizeof(unsigned) == TB_BUDGET / 4, "the list table fills a quarter of the scratch at most");

struct TsTile { unsigned l0, len, first, count; };        // the list (start in the table's index area, length), first sorted user, users <= TB_TU

struct TsArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // chunk position -> row of A
    const unsigned* perm;             // sorted user -> chunk position
    const TsTile* tiles;
    const unsigned* lists;            // the table's indices, one row after the other
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users, by chunk position
    real_t* part_score;               // [chunk position][nslices][n_top]
    unsigned* part_ix;
};

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void topn_shared_kernel(TsArgs a)
{
    extern __shared__ __align__(16) unsigned char ts_smem[];
    T* As = (T*)ts_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    unsigned char* sel_lds = (unsigned char*)(Bs + TB_TJ * TB_KS);
    unsigned* upos = (unsigned*)(sel_lds + tb_select_bytes(a.cap));   // [TB_TU] the user's position in the chunk

    const TsTile tile = a.tiles[blockIdx.x];
    const unsigned len = tile.len;
    const unsigned ntiles = (len + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    if (blockIdx.y > 0 && tile0 >= ntiles) return;        // (the whole workgroup, before any barrier: the merge knows this user's slices)
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned* lst = a.lists + tile.l0;

    if (threadIdx.x < TB_TU) upos[threadIdx.x] = threadIdx.x < tile.count ? a.perm[tile.first + threadIdx.x] : 0u;
    TbSelect<T, TbPrunePlain> sel;
    sel.init(sel_lds, a.cap, a.n_top, TbPrunePlain(), [&](unsigned row) { return row < tile.count ? a.users[upos[row]] : TB_NONE; });   // (row: the thread's own)

    const unsigned col = threadIdx.x & 15;
    auto user_row = [&](int row) { return sel.user_row(row); };
    // tile row `row` of the step at list position p: the list's entry there, none past its end
    auto item_rows = [lst, len](unsigned p) {
        return [lst, len, p](int row) { const unsigned q = p + (unsigned)row; return q < len ? (long long)lst[q] : -1ll; };
    };
    auto pos_of = [upos](unsigned uu) { return upos[uu]; };   // a tile row's position in the chunk

    // this lane's four candidates of a step, fetched one step ahead like the rows they name
    unsigned j_next[4];
    auto fetch_items = [&](unsigned p) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned q = p + 16 * t + col;
            j_next[t] = q < len ? lst[q] : TB_NONE;
        }
    };
    if (tile0 < tile1) fetch_items(tile0 * TB_TJ);

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, item_rows, [&](T (&acc)[4][4], unsigned p_base) {
        unsigned j_cur[4];
#pragma unroll
        for (int t = 0; t < 4; t++) j_cur[t] = j_next[t];
        if (p_base + TB_TJ < tile1 * TB_TJ) fetch_items(p_base + TB_TJ);
#pragma unroll
        for (int t = 0; t < 4; t++)   // (in range by position: a phantom row past the list's end scores 0 like any zero row)
            sel.pass(acc[t], j_cur[t], p_base + 16 * t + col < len, a.excl, pos_of);
    });
    sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);
}

// One wave per chunk position: the best n_top of the user's ns[u] <= nslices sorted partial lists, [position][nslices][n_top].
__global__ __launch_bounds__(64) void topn_shared_merge_kernel(const real_t* part_score, const unsigned* part_ix, const unsigned* ns, unsigned nslices,
                                                               unsigned n_top, real_t* out_score, unsigned* out_ix)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX];
    const unsigned u = blockIdx.x, n = ns[u];
    const size_t o = (size_t)u * nslices * n_top;
    real_t* o_score = out_score + (size_t)u * n_top;
    unsigned* o_ix = out_ix + (size_t)u * n_top;
    tb_merge_lists(ms, mj, part_score + o, part_ix + o, n, n_top, o_score, o_ix);
    tb_merge_pad(mj, n, n_top, o_score, o_ix);   // a short row: ranks that no real entry reached
}

// The one scratch allocation of a call: the list table and what a chunk of users needs, in bytes from the start.
struct TsLayout {
    size_t chunk_users;      // users per chunk
    size_t cell_cap;         // indices of the list table
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t part_rows;        // (user, slice) rows of a chunk's partial lists
    size_t lists, users, perm, ns, tiles, ex_indptr, ex_indices, part_score, part_ix, out_score, out_ix, total;
    TsLayout(size_t n_users, size_t n_cells, size_t n_top, size_t dimB)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::max<size_t>(dimB, 1);
        const size_t first = std::min(n_users, TB_CHUNK_USERS_MAX);
        cell_cap = std::min(TS_MAX_CELLS, std::max<size_t>(n_cells, 1));                  // a quarter of the budget at most
        idx_cap = std::min(TB_BUDGET / 2 / sizeof(unsigned), first * dimB);               // section 1f's: half of it  (no overflow: 2^18 x 2^31)
        const size_t row = n_top * (R + 4);
        // a user has at most min(TB_MERGE_MAX / n_top, item tiles of the longest list) slices, a chunk about TB_TU x TS_TARGET_WGS + users
        // rows; the run cuts a chunk's slices down to what is here
        const size_t most = std::min(TB_MERGE_MAX / n_top, pmf_ceil_div(std::min(cell_cap, dimB), (size_t)TB_TJ));
        part_rows = std::min({ TS_PART_BYTES / row, first * most, (size_t)TB_TU * TS_TARGET_WGS + first });
        const size_t rest = TB_BUDGET - (cell_cap + idx_cap) * sizeof(unsigned) - part_rows * row - 512;   // (512: alignment of the eleven parts)
        const size_t per_user = 4 * sizeof(unsigned) + sizeof(TsTile) + row;              // (a tile per user at worst)
        chunk_users = std::max<size_t>(std::min({ rest / per_user, TB_CHUNK_USERS_MAX, n_users }), 1);
        TbTake take;
        lists = take(cell_cap * sizeof(unsigned));
        users = take(chunk_users * sizeof(unsigned));
        perm = take(chunk_users * sizeof(unsigned));
        ns = take(chunk_users * sizeof(unsigned));
        tiles = take(chunk_users * sizeof(TsTile));
        ex_indptr = take((chunk_users + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        part_score = take(part_rows * n_top * R);
        part_ix = take(part_rows * n_top * sizeof(unsigned));
        out_score = take(chunk_users * n_top * R);
        out_ix = take(chunk_users * n_top * sizeof(unsigned));
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_shared_scratch_bytes(size_t n_users, size_t n_lists, size_t n_cells, size_t n_top, size_t dimB, size_t k)
{
    (void)n_lists;   // (a tile carries its list's place in the table: no row pointers go to the device)
    (void)k;         // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TsLayout(n_users, n_cells, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_shared_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                 const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of,
                                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || list_indptr == nullptr || list_of == nullptr || n_lists == 0) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA || (size_t)list_of[i] >= n_lists) return 2;
    if ((size_t)list_indptr[n_lists] - (size_t)list_indptr[0] > TS_MAX_CELLS) return 2;   // (the table as a whole, before an index is read)
    if (!tb_rows_ok(list_indptr, list_indices, n_lists, dimB, TS_MAX_CELLS)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_shared_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                               const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* list_indptr,
                               const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of, PmfTopnSeen* seen,
                               const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap,
                               sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t l_base = (size_t)list_indptr[0];
    const size_t n_cells = (size_t)list_indptr[n_lists] - l_base;
    const TsLayout L(n_users, n_cells, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, TS_UPOS_BYTES);
    const size_t lds = tb_lds_bytes(cap, TS_UPOS_BYTES);
    auto kern = topn_shared_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));

    TsArgs a;
    std::vector<unsigned> hl, hu, hperm, hns, hp, hx, hix, touched, count;
    std::vector<TsTile> tiles;
    try {
        // the table: once per call, narrowed to 32 bits
        hl.resize(n_cells);
        for (size_t p = 0; p < n_cells; p++) hl[p] = (unsigned)list_indices[l_base + p];
        count.assign(n_lists, 0u);   // users of each list in the chunk at hand; all zero between chunks
    } catch (const std::bad_alloc&) { return 1; }
    TB_TRY(pmf_upload(base + L.lists, hl.data(), n_cells * sizeof(unsigned), stream));
    auto list_len = [&](size_t g) { return (size_t)list_indptr[g + 1] - (size_t)list_indptr[g]; };

    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users consecutive users whose exclusion lists fit the index area together
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;

        // the users in order of their list (a stable counting sort over the lists the chunk refers to), cut into tiles of one list each
        touched.clear();
        for (size_t i = 0; i < nu; i++) {
            const size_t g = (size_t)list_of[u0 + i];
            if (count[g]++ == 0) touched.push_back((unsigned)g);
        }
        std::sort(touched.begin(), touched.end());
        tiles.clear();
        size_t first = 0, max_len = 0;
        for (const unsigned g : touched) {
            const size_t c = count[g], len = list_len(g);
            for (size_t f = 0; f < c; f += TB_TU)
                tiles.push_back({ (unsigned)((size_t)list_indptr[g] - l_base), (unsigned)len, (unsigned)(first + f), (unsigned)std::min<size_t>(TB_TU, c - f) });
            count[g] = (unsigned)first;   // (from here on: where the list's next user goes)
            first += c;
            max_len = std::max(max_len, len);
        }
        hperm.resize(nu);
        for (size_t i = 0; i < nu; i++) hperm[count[(size_t)list_of[u0 + i]]++] = (unsigned)i;
        for (const unsigned g : touched) count[g] = 0;

        // slices: one length per launch, from the longest list; a user has as many as its own list reaches
        const size_t slice_cap = std::max<size_t>(1, std::min(TB_MERGE_MAX / n_top, L.part_rows / nu));   // (the merge kernel's LDS; the partial lists' area)
        const TbSlices sl = tb_slices(tiles.size(), std::max<size_t>(max_len, 1), TS_TARGET_WGS, slice_cap);
        const size_t nslices = sl.nslices;
        if (tiles.size() > L.chunk_users || (nslices > 1 && nu * nslices > L.part_rows)) return 1;   // (cannot happen: TsLayout sizes the areas for any chunk)
        TB_TRY(pmf_upload(base + L.perm, hperm.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.tiles, tiles.data(), tiles.size() * sizeof(TsTile), stream));
        if (nslices > 1) {
            hns.resize(nu);
            for (size_t i = 0; i < nu; i++)
                hns[i] = (unsigned)std::max<size_t>(1, pmf_ceil_div(pmf_ceil_div(list_len((size_t)list_of[u0 + i]), (size_t)TB_TJ), sl.tiles_per_slice));
            TB_TRY(pmf_upload(base + L.ns, hns.data(), nu * sizeof(unsigned), stream));
        }
        a.A = dA;
        a.B = dB;
        a.users = (const unsigned*)(base + L.users);
        a.perm = (const unsigned*)(base + L.perm);
        a.tiles = (const TsTile*)(base + L.tiles);
        a.lists = (const unsigned*)(base + L.lists);
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.cap = (unsigned)cap;
        a.nslices = (unsigned)nslices;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        // (one slice: its sorted lists are the results)
        a.part_score = (real_t*)(base + (nslices == 1 ? L.out_score : L.part_score));
        a.part_ix = (unsigned*)(base + (nslices == 1 ? L.out_ix : L.part_ix));
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size(), (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            hipLaunchKernelGGL(topn_shared_merge_kernel, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix,
                               (const unsigned*)(base + L.ns), (unsigned)nslices, (unsigned)n_top, (real_t*)(base + L.out_score),
                               (unsigned*)(base + L.out_ix));
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score), hix, out_ix, out_score, stream)) return 1;
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_shared(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                           size_t n_top, const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of,
                           const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_shared_check(users, n_users, n_top, dimA, dimB, (size_t)k, list_indptr, list_indices, n_lists, list_of,
                                                    excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_shared_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, list_indptr, list_indices,
                                                           n_lists, list_of, nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix,
                                                           out_score);
                     });
}

}  // extern "C"
