// rank_sampled.hip -- sampled evaluation in one pass (include/poismf_hip.h, section 1u): for many users at once, m negatives are
// drawn as section 1t draws them (avoiding E(u) and the user's own held-out row), scored, and each held-out item is ranked among them
// and the user's other held-out items -- section 1j's ranks for I(u) = S(u) united with T(u), without the sample ever leaving LDS:
// no kernel here writes or reads an m-wide row in global memory, nothing is sorted, and only ranks and per-user integers come down.
//
//   rank_threshold_kernel<false>  (tb_rank.hpp) a held-out cell's score, and whether its item is in E(u).
//   rank_order_kernel             (tb_rank.hpp) the user's valid thresholds best first.  A threshold's place in that order IS the number
//                                 of held-out items before it, so T(u) is never gathered as candidates.
//   rank_sampled_kernel           one work item per user, in three steps:
//       draw    ONE wave runs sn_draw_row (sn_draw.hpp: the sampler's own rounds of 64 Philox blocks, table and cut); its admissibility
//               test is tb_excluded plus a binary search in the user's ascending held-out row.  The accepted items are appended to a
//               list in LDS, unsorted: a rank does not depend on the list's order.  count, draws and N(u) = count + valid held-out
//               cells are written here; a user with no valid held-out cell is done and has read no row of B.
//       score   the list feeds tb_gather.hpp's gather and ti_pass chain, 64 candidates a pass, the rows of B in 16-byte pieces.  Each
//               score is searched (rb_first_beaten) in the user's ordered thresholds in LDS and adds 1 to the LDS bin of the first
//               one it comes before.  Every sampled item is admissible by construction: no exclusion test here.
//       count   the running sums over the bins plus each threshold's own place are the ranks' counts (`dense`); rank_finish_kernel
//               puts them in the caller's order.  The user's bins belong to its own waves only: integer adds in LDS, no global
//               atomics.  A user with more than POISMF_HIP_RANK_INCLUDE_GROUP valid held-out items searches them in global memory
//               and adds to the global difference array that rank_finish_kernel sums, as section 1j does.
//   rank_finish_kernel<true>      (tb_rank.hpp) rank = count + running sum of the difference array; RANK_EXCLUDED for cells in E(u).
//
// The split.  The draw of one user is sequential in rounds and belongs to one wave; the scoring of its list is not.
//   m <= SN_SMALL_M  four waves per workgroup, one user each, sharing nothing and meeting at no workgroup barrier (the sampler's small
//                    instance, rank_include_kernel's shape): at most four passes of scoring per user, not worth a second wave.
//   above            one workgroup of RS_TEAM = 3 waves per user: wave 0 draws while wave 2 stages the user's row of A and its
//                    thresholds; after ONE barrier the waves score passes w, w + 3, ... of the LDS list, each through a tile of its
//                    own, into the user's one set of bins (LDS integer adds commute); after a second barrier wave 0 sums.  Three
//                    waves, not four, because of LDS: see below.
// LDS per user: a gather tile per wave (17 KB each), the list (m entries), the row of A, 128 thresholds and bins.  The table of the
// draw (2 m slots and more, 32 KB at m = 4096) and the coarse index of the weighted draw (8 KB, a copy per user: it is read from L2
// once) live INSIDE the tiles: the draw is over before the first row of B is staged.  That leaves 20 KB per user in the small instance
// and 69 KB at m = 4096 with three waves, two workgroups per CU either way at k = 50 (fp32; the static_asserts below); a fourth
// wave's tile would leave one.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds
// the prefix sums and a chunk (RsLayout; poismf_hip_rank_sampled_scratch_bytes).  Per chunk the users, stream ids, held-out rows and
// exclusion lists go up and the ranks and three integers per user come down.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_rank.hpp"
#include "tb_batch.hpp"
#include "sn_draw.hpp"
#include "cores.hpp"

namespace {

constexpr int RS_WAVES = 4;                               // small instance: users of a workgroup, one wave each
constexpr int RS_TEAM = 3;                                // large instance: waves of a workgroup's one user
constexpr unsigned RS_G = POISMF_HIP_RANK_INCLUDE_GROUP;  // thresholds (and bins) a user keeps in LDS
constexpr size_t RS_TILE = 64 * (size_t)TI_SLOT;          // one wave's gather tile
static_assert(RS_G == 128, "the running sums of a wave: two bins per lane");

struct RsArgs {
    RbArgs r;                             // the chunk: factors, held-out cells, thresholds, counters (r.incl / r.iptr unused)
    SnDraw d;                             // section 1t's draw
    const unsigned long long* streams;    // [chunk users] stream ids
    unsigned list_cap;                    // list entries per user: m rounded up to whole passes
    unsigned* cnt;                        // [chunk users] |S(u)|
    unsigned* draws;                      // [chunk users]
};

// tiles, list, row of A (zero padded to four columns), thresholds (score, item), bins, and 16 bytes for the count
__host__ __device__ constexpr size_t rs_user_lds(size_t k, size_t waves, size_t list_cap)
{
    return waves * RS_TILE + list_cap * sizeof(unsigned) + ((k + 3) & ~(size_t)3) * TI_R + RS_G * (TI_R + 2 * sizeof(unsigned)) + 16;
}
constexpr size_t rs_list_cap(size_t m) { return m <= SN_SMALL_M ? SN_SMALL_M : (m + 63) & ~(size_t)63; }
// two workgroups per CU (160 KB of LDS) at k = 50: the large instance in both precisions, the small one in fp32 (fp64: 163 KB, one)
static_assert(2 * rs_user_lds(50, RS_TEAM, rs_list_cap(SN_MAX_M)) <= 160 * 1024, "two workgroups of the longest row per CU at k = 50");
static_assert(sizeof(real_t) == 8 || 2 * RS_WAVES * rs_user_lds(50, 1, SN_SMALL_M) <= 160 * 1024, "two workgroups of the small instance per CU at k = 50");
// the draw's table and coarse index fit the tiles they borrow
static_assert(SN_SMALL_SLOTS * 4 + SN_COARSE * 8 <= RS_TILE && 2 * SN_MAX_M * 4 + SN_COARSE * 8 <= RS_TEAM * RS_TILE, "table and coarse index inside the tiles");
static_assert(RS_WAVES * rs_user_lds(TB_K_MAX, 1, SN_SMALL_M) <= 160 * 1024 && rs_user_lds(TB_K_MAX, RS_TEAM, rs_list_cap(SN_MAX_M)) <= 160 * 1024, "a workgroup fits at every k");

template <int WAVES, bool TEAM, bool WEIGHTED> __global__ __launch_bounds__(64 * WAVES) void rank_sampled_kernel(RsArgs a)
{
    extern __shared__ __align__(16) unsigned char rs_smem[];
    constexpr unsigned NW = TEAM ? WAVES : 1;   // waves of one user
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned wl = TEAM ? wave : 0;        // this wave among its user's
    const unsigned ui = TEAM ? blockIdx.x : blockIdx.x * WAVES + wave;
    if (ui >= a.r.n_users) return;   // (TEAM: the whole workgroup; otherwise the waves share nothing and meet at no barrier)
    const int k = a.r.k;
    const int ka = (k + 3) & ~3;
    unsigned char* tiles = rs_smem + (TEAM ? 0 : wave * rs_user_lds((size_t)k, 1, a.list_cap));   // [NW][64][TI_SLOT]; during the draw: table, coarse index
    unsigned* lst = (unsigned*)(tiles + NW * RS_TILE);             // [list_cap] S(u) in the order of its draws
    real_t* As = (real_t*)(lst + a.list_cap);                      // [ka] the user's row, zero padded
    real_t* Ts = As + ka;                                          // [RS_G] the user's thresholds, best first: score ...
    unsigned* Tj = (unsigned*)(Ts + RS_G);                         // ... and item
    unsigned* bins = Tj + RS_G;                                    // [RS_G] sampled items whose first beaten threshold is this one
    unsigned* meta = bins + RS_G;                                  // [0]: |S(u)|
    auto sync = [] { if (TEAM) __syncthreads(); else tb_wave_sync(); };

    const unsigned arow = a.r.arow[ui];
    const unsigned t0 = a.r.tptr[ui], t1 = a.r.tptr[ui + 1], nv = a.r.nvalid[ui];
    const bool big = nv > RS_G;             // (uniform) the thresholds stay in global memory
    const unsigned n = big ? 0u : nv;       // thresholds in LDS

    // ---- draw: one wave ----
    if (wl == 0) {
        unsigned* tab = (unsigned*)tiles;
        unsigned long long* cs = (unsigned long long*)(tiles + (sizeof(unsigned) << a.d.log_slots));
        if (WEIGHTED)
            for (unsigned t = lane; t < a.d.n_coarse; t += 64) cs[t] = a.d.coarse[t];   // (sn_draw_row's first wave sync comes before any read)
        unsigned draws;
        const unsigned count = sn_draw_row<WEIGHTED>(a.d, cs, tab, lst, a.streams[ui], lane, [&](unsigned j) {
            return !tb_excluded(a.r.excl, ui, arow, j) && !tb_sorted_has(a.r.cell_item, t0, t1, j);   // E(u), then T(u): a row of the caller's, ascending
        }, draws);
        if (lane == 0) {
            a.cnt[ui] = count;
            a.draws[ui] = draws;
            a.r.n_adm[ui] = count + nv;
            meta[0] = count;
        }
    }
    if (nv == 0) return;   // (uniform for the user's waves, none of which has met a barrier) nothing to rank: no row of B is read

    // ---- the user's row and thresholds: the last wave, beside the draw ----
    if (wl == NW - 1) {
        const real_t* Au = a.r.A + (size_t)arow * (size_t)k;
        for (int c = (int)lane; c < ka; c += 64) As[c] = c < k ? Au[c] : (real_t)0;
        for (unsigned i = lane; i < RS_G; i += 64) {
            Ts[i] = i < n ? a.r.s_score[t0 + i] : (real_t)0;
            Tj[i] = i < n ? a.r.s_item[t0 + i] : 0u;
            bins[i] = 0;
        }
    }
    sync();   // the list is complete, the table is dead: the tiles are the gather's

    // ---- score: wave wl takes passes wl, wl + NW, ... of the list ----
    const unsigned count = meta[0];
    const unsigned npass = (count + 63) / 64;
    const unsigned mine = npass > wl ? (npass - wl + NW - 1) / NW : 0u;
    const TiGather g = { (const char*)a.r.B, tiles + wl * RS_TILE, k, lane >> 2, lane & 3 };
    auto item_of = [&](unsigned q) {   // this lane's candidate of the wave's q-th pass
        const unsigned e = (wl + q * NW) * 64 + lane;
        return e < count ? lst[e] : TB_NONE;
    };
    ti_u32x4 pre[TI_NI];
    unsigned j_cur = item_of(0), j_nxt = item_of(1);
    if (mine) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);
    for (unsigned q = 0; q < mine; q++) {
        const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, q, mine);
        if (j_cur != TB_NONE) {
            if (big) {
                const unsigned pos = rb_first_beaten(a.r.s_score + t0, a.r.s_item + t0, nv, s, j_cur);
                if (pos < nv) atomicAdd(&a.r.corr[t0 + pos], 1u);   // (global, integer)
            } else {
                const unsigned pos = rb_first_beaten(Ts, Tj, n, s, j_cur);
                if (pos < n) atomicAdd(&bins[pos], 1u);             // (LDS, integer)
            }
        }
        j_cur = j_nxt;
        j_nxt = item_of(q + 2);
    }
    sync();

    // ---- count: a sampled item before threshold i is before every later one; i held-out items stand before threshold i ----
    if (wl != 0) return;
    if (big) {
        for (unsigned i = lane; i < nv; i += 64) a.r.dense[t0 + i] = i;
        return;
    }
    unsigned run0 = 0, run1 = 0;   // of thresholds lane and 64 + lane
    for (unsigned q = 0; q < n; q++) {
        const unsigned b = bins[q];   // (one address for the wave: a broadcast)
        run0 += q <= lane ? b : 0u;
        run1 += q <= 64 + lane ? b : 0u;
    }
    if (lane < n) a.r.dense[t0 + lane] = lane + run0;
    if (64 + lane < n) a.r.dense[t0 + 64 + lane] = 64 + lane + run1;
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct RsLayout {
    size_t chunk_users;      // users per chunk
    size_t cell_cap;         // held-out cells a chunk may carry
    size_t excl_cap;         // exclusion indices a chunk may carry
    size_t C, coarse, users, streams, tptr, ex_indptr, nvalid, n_adm, cnt, draws, cell_row, cell_item, cell_score, cell_excl, s_score, s_item,
        s_origin, dense, corr, rank, ex_indices, total;
    RsLayout(size_t n_users, size_t n_test, size_t dimB, bool weighted)
    {
        const size_t R = sizeof(real_t), U = sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_test = std::max<size_t>(n_test, 1);
        dimB = std::max<size_t>(dimB, 1);
        // the prefix sums (at most 128 MiB), a quarter of the budget at most for the exclusion lists (section 1t's), the users' own parts
        // -- stream id and seven integers -- and the cells from the rest: eight index arrays, two of scores
        const size_t c_bytes = weighted ? pmf_round_up(dimB * sizeof(unsigned long long), 32) + SN_COARSE * sizeof(unsigned long long) : 0;
        const size_t excl_max = TB_BUDGET / 4 / U;
        chunk_users = std::min(n_users, TB_CHUNK_USERS_MAX);
        excl_cap = chunk_users <= excl_max / dimB ? chunk_users * dimB : excl_max;
        const size_t per_user = sizeof(unsigned long long) + 7 * U, per_cell = 8 * U + 2 * R;
        const size_t rest = TB_BUDGET - c_bytes - excl_cap * U - per_user * chunk_users - 32 * 24;   // (32: alignment of each of the parts, two spare row pointers)
        cell_cap = std::min(n_test, rest / per_cell);
        TbTake take;
        C = take(weighted ? dimB * sizeof(unsigned long long) : 0);
        coarse = take(weighted ? SN_COARSE * sizeof(unsigned long long) : 0);
        users = take(chunk_users * U);
        streams = take(chunk_users * sizeof(unsigned long long));
        tptr = take((chunk_users + 1) * U);
        ex_indptr = take((chunk_users + 1) * U);
        nvalid = take(chunk_users * U);
        n_adm = take(chunk_users * U);
        cnt = take(chunk_users * U);
        draws = take(chunk_users * U);
        cell_row = take(cell_cap * U);
        cell_item = take(cell_cap * U);
        cell_score = take(cell_cap * R);
        cell_excl = take(cell_cap * U);
        s_score = take(cell_cap * R);
        s_item = take(cell_cap * U);
        s_origin = take(cell_cap * U);
        dense = take(cell_cap * U);
        corr = take(cell_cap * U);
        rank = take(cell_cap * U);
        ex_indices = take(excl_cap * U);
        total = take.o;
    }
};
// the least a chunk's cells get -- the prefix sums of 2^24 items, a full exclusion area and every user of a chunk present -- holds the
// longest held-out row a call accepts
static_assert((TB_BUDGET - SN_MAX_ITEMS * 8 - SN_COARSE * 8 - TB_BUDGET / 4 - (8 + 7 * sizeof(unsigned)) * TB_CHUNK_USERS_MAX - 32 * 24) /
                      (8 * sizeof(unsigned) + 2 * sizeof(real_t)) >= RB_ROW_MAX,
              "one held-out row fits a chunk");
static_assert(SN_MAX_ITEMS <= TB_BUDGET / 4 / sizeof(unsigned), "the longest exclusion row fits a chunk");

template <int WAVES, bool TEAM, bool WEIGHTED> hipError_t rs_launch(const RsArgs& a, hipStream_t stream)
{
    const size_t lds = TEAM ? rs_user_lds((size_t)a.r.k, WAVES, a.list_cap) : WAVES * rs_user_lds((size_t)a.r.k, 1, a.list_cap);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rank_sampled_kernel<WAVES, TEAM, WEIGHTED>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const unsigned blocks = TEAM ? a.r.n_users : (unsigned)pmf_ceil_div(a.r.n_users, WAVES);
    hipLaunchKernelGGL((rank_sampled_kernel<WAVES, TEAM, WEIGHTED>), dim3(blocks), dim3(64 * WAVES), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t poismf_hip_rank_sampled_scratch_bytes(size_t n_users, size_t n_test_cells, size_t m, size_t dimB, size_t k, int weighted)
{
    (void)m;   // (the sampled rows live in LDS, as the factors' chunks do: no part of the scratch depends on m or k)
    (void)k;
    return RsLayout(n_users, n_test_cells, dimB, weighted != 0).total;
}

// The argument checks of both entry points, sections 1j's and 1t's together: 0, or 2.  No device call.
int poismf_hip_rank_sampled_check(const sparse_ix* users, size_t n_users, size_t m, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                  const sparse_ix* test_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                  const uint32_t* item_weight)
{
    if (k < 1 || k > TB_K_MAX || dimA < 1 || dimA > 0x7fffffffull || test_indptr == nullptr) return 2;
    if (const int rc = poismf_hip_sample_negatives_check(users, n_users, m, dimA, dimB, excl_indptr, excl_indices, item_weight)) return rc;
    return tb_rows_ok(test_indptr, test_indices, n_users, dimB, RB_ROW_MAX) ? 0 : 2;
}

// ---- core on device-resident factors (cores.hpp) ----
int poismf_hip_rank_sampled_core(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                 const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t m,
                                 uint64_t seed, PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                 const uint32_t* item_weight, void** d_scratch, size_t* scratch_cap, unsigned int* out_rank,
                                 unsigned int* out_n_adm, unsigned int* out_count, unsigned int* out_draws)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const bool weighted = item_weight != nullptr;
    const size_t n_test = (size_t)test_indptr[n_users] - (size_t)test_indptr[0];
    const RsLayout L(n_users, n_test, dimB, weighted);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    RsArgs a = {};
    RbArgs& r = a.r;
    a.d = sn_draw_of(m, dimB, seed);
    a.list_cap = (unsigned)rs_list_cap(m);
    a.streams = (const unsigned long long*)(base + L.streams);
    a.cnt = (unsigned*)(base + L.cnt);
    a.draws = (unsigned*)(base + L.draws);
    if (weighted) TB_TRY(sn_stage_weights(a.d, item_weight, dimB, base + L.C, base + L.coarse, stream));
    r.A = dA;
    r.B = dB;
    r.k = (int)k;
    r.dimB = (unsigned)dimB;
    r.arow = (const unsigned*)(base + L.users);
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

    std::vector<unsigned> hu, hp, hx, htp, hrow, hitem;
    std::vector<unsigned long long> hs;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: the users whose held-out cells fit the cell area, then tb_stage_chunk's cut by users and exclusion indices
        size_t fit = u0, nc = 0;
        while (fit < n_users && fit - u0 < L.chunk_users) {
            const size_t cells = (size_t)test_indptr[fit + 1] - (size_t)test_indptr[fit];
            if (fit > u0 && nc + cells > L.cell_cap) break;
            nc += cells;
            fit++;
        }
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, r.excl, u0, fit, L.chunk_users, L.excl_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L), hu,
                           hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0, c_base = (size_t)test_indptr[u0];
        nc = (size_t)test_indptr[u1] - c_base;
        if (nc > L.cell_cap) return 1;   // (cannot happen: the checks bound a single row by the cell area)
        hs.resize(nu);
        htp.resize(nu + 1);
        hrow.resize(nc);
        hitem.resize(nc);
        for (size_t i = 0; i < nu; i++) {
            hs[i] = (unsigned long long)(size_t)users[u0 + i];
            const size_t p0 = (size_t)test_indptr[u0 + i] - c_base, p1 = (size_t)test_indptr[u0 + i + 1] - c_base;
            htp[i] = (unsigned)p0;
            for (size_t p = p0; p < p1; p++) {
                hrow[p] = (unsigned)i;
                hitem[p] = (unsigned)test_indices[c_base + p];
            }
        }
        htp[nu] = (unsigned)nc;
        TB_TRY(pmf_upload(base + L.streams, hs.data(), nu * sizeof(unsigned long long), stream));
        TB_TRY(pmf_upload(base + L.tptr, htp.data(), (nu + 1) * sizeof(unsigned), stream));
        TB_TRY(hipMemsetAsync(base + L.nvalid, 0, nu * sizeof(unsigned), stream));
        r.n_users = (unsigned)nu;
        r.n_cells = (unsigned)nc;
        if (nc > 0) {
            TB_TRY(pmf_upload(base + L.cell_row, hrow.data(), nc * sizeof(unsigned), stream));
            TB_TRY(pmf_upload(base + L.cell_item, hitem.data(), nc * sizeof(unsigned), stream));
            TB_TRY(hipMemsetAsync(base + L.corr, 0, nc * sizeof(unsigned), stream));
            const unsigned cell_blocks = (unsigned)pmf_ceil_div(nc, 256);
            hipLaunchKernelGGL(rank_threshold_kernel<false>, dim3(cell_blocks), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(rank_order_kernel, dim3(cell_blocks), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
        }
        if (m <= SN_SMALL_M) TB_TRY((weighted ? rs_launch<RS_WAVES, false, true>(a, stream) : rs_launch<RS_WAVES, false, false>(a, stream)));
        else TB_TRY((weighted ? rs_launch<RS_TEAM, true, true>(a, stream) : rs_launch<RS_TEAM, true, false>(a, stream)));
        if (nc > 0) {
            hipLaunchKernelGGL(rank_finish_kernel<true>, dim3((unsigned)pmf_ceil_div(nu, 256)), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
            TB_TRY(pmf_download(out_rank + c_base, base + L.rank, nc * sizeof(unsigned), stream));
        }
        TB_TRY(pmf_download(out_n_adm + u0, base + L.n_adm, nu * sizeof(unsigned), stream));
        if (out_count != nullptr) TB_TRY(pmf_download(out_count + u0, base + L.cnt, nu * sizeof(unsigned), stream));
        if (out_draws != nullptr) TB_TRY(pmf_download(out_draws + u0, base + L.draws, nu * sizeof(unsigned), stream));
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_rank_sampled(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t m, uint64_t seed, const sparse_ix* excl_indptr,
                            const sparse_ix* excl_indices, const uint32_t* item_weight, unsigned int* out_rank, unsigned int* out_n_adm,
                            unsigned int* out_count, unsigned int* out_draws)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_sampled_check(users, n_users, m, dimA, dimB, (size_t)k, test_indptr, test_indices, excl_indptr, excl_indices,
                                                     item_weight))
        return rc;
    // (tb_dropin's copy of B carries the 16 bytes of slack the gather may read past a row)
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_rank_sampled_core(st, dA, dB, dimB, (size_t)k, compact, users, n_users, test_indptr, test_indices, m, seed,
                                                             nullptr, excl_indptr, excl_indices, item_weight, d_scratch, scratch_cap, out_rank,
                                                             out_n_adm, out_count, out_draws);
                     });
}

}  // extern "C"
