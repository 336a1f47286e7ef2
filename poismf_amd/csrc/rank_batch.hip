// rank_batch.hip -- batched exact ranks (include/poismf_hip.h, section 1g): for many users at once, the 0-based position of each
// held-out item in the user's complete ranked list under the total order "score descending, item index ascending", exclusion sets
// left out.  score(u, j) is section 1f's: the k-ordered fused chain, bit for bit what pair_dot_kernel (serve.hip) computes.
//
// rank(u, t) = #{j in 0..dimB-1 before t} - #{e in E(u) before t}: a dense count over every item and a sparse correction.
//
//   (tb_rank.hpp, shared with rank_include.hip: rank_threshold_kernel, rank_order_kernel and rank_finish_kernel)
//   rank_threshold_kernel  one thread per held-out cell: its score with the scalar chain (the "threshold"), and whether it is in E(u).
//   rank_order_kernel      one thread per cell: its position among the user's cells (valid ones best first under the total order, cells
//                          in E(u) behind them), by counting -- quadratic in a row's length, hence POISMF_HIP_RANK_BATCH_MAX_ROW.
//   rank_tile_kernel       the users x items tile of tb_tile.hpp with a counting epilogue.  A row of the tile is a GROUP: up to RB_G
//                          consecutive thresholds of one user (a user with more occupies several rows; ranks of different thresholds
//                          are independent).  LDS holds the groups' thresholds and RB_G integer bins per row, registers the group's
//                          best and worst threshold.  A score that does not come before the worst threshold dies in registers; one
//                          before the best adds to a register counter; one in between is compared with the thresholds between them
//                          (read from LDS once for the lane's four scores of that row) and adds 1 to the bin of the first threshold
//                          it comes before (LDS integer add).  At the end a row's running sum over its bins
//                          is the slice's count for each threshold; slices add theirs with integer atomics (order cannot matter).
//                          The tile's score of item t has the bits of t's threshold (tests/test_gpu_rank_batch.py), so t never
//                          comes before itself.
//   rank_excl_kernel       one wave per user over E(u) (the batch's list, then the resident row minus what the list already had):
//                          the item's score with the scalar chain, a binary search in the user's ordered thresholds, +1 in a
//                          difference array at the first threshold it comes before; and N(u) = dimB - |E(u)|.
//   rank_finish_kernel     one thread per user: rank = dense count - running sum of the difference array, written at the cell's
//                          place in the caller's order; POISMF_HIP_RANK_EXCLUDED for cells in E(u).
//
// All counting is in integers; no float atomics.  The host side cuts the batch into chunks of users so that ONE scratch allocation of
// at most POISMF_HIP_RANK_BATCH_BUDGET_MB holds a chunk (RbLayout; poismf_hip_rank_batch_scratch_bytes reports its size).
#include <cstring>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_rank.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int RB_G = 32;                                  // thresholds per row of the tile
constexpr int RB_GS = RB_G + 1;                           // LDS row stride of thresholds and bins (rows 4 apart fall on banks 4 apart)
constexpr size_t RB_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many
constexpr size_t RB_CHUNK_USERS_MAX = 262144;
constexpr size_t RB_BUDGET = (size_t)POISMF_HIP_RANK_BATCH_BUDGET_MB << 20;

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void rank_tile_kernel(RbArgs a)
{
    extern __shared__ __align__(16) unsigned char rb_smem[];
    T* As = (T*)rb_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    T* Ts = Bs + TB_TJ * TB_KS;                           // [TB_TU][RB_GS] a group's thresholds, best first: score ...
    unsigned* Tj = (unsigned*)(Ts + TB_TU * RB_GS);       // ... and item
    unsigned* bins = Tj + TB_TU * RB_GS;                  // [TB_TU][RB_GS] scores whose first beaten threshold is this one
    unsigned* uid = bins + TB_TU * RB_GS;                 // [TB_TU] row of A, TB_NONE for a row without thresholds
    unsigned* gn = uid + TB_TU;                           // [TB_TU] thresholds in the group
    unsigned* gs = gn + TB_TU;                            // [TB_TU] its first ordered entry

    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned g_base = blockIdx.x * TB_TU;
    if (tid < TB_TU) {
        const unsigned g = g_base + tid;
        unsigned u = TB_NONE, n = 0, st = 0;
        if (g < a.ngroups) {
            const unsigned row = a.grow[g];
            st = a.gstart[g];
            const unsigned off = st - a.tptr[row], nv = a.nvalid[row];
            if (nv > off) n = nv - off < (unsigned)RB_G ? nv - off : (unsigned)RB_G;
            if (n > 0) u = a.arow[row];
        }
        uid[tid] = u;
        gn[tid] = n;
        gs[tid] = st;
    }
    __syncthreads();
    for (unsigned e = tid; e < (unsigned)(TB_TU * RB_G); e += TB_WG) {
        const unsigned row = e / RB_G, i = e % RB_G;
        const bool in = i < gn[row];
        Ts[row * RB_GS + i] = in ? a.s_score[gs[row] + i] : (T)0;
        Tj[row * RB_GS + i] = in ? a.s_item[gs[row] + i] : 0u;
        bins[row * RB_GS + i] = 0;
    }
    __syncthreads();

    const unsigned ntiles = (a.dimB + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned col = lane & 15, quad = lane >> 4;
    const unsigned urow0 = 16 * wave + 4 * quad;          // this lane's four rows are urow0 .. urow0 + 3
    auto user_row = [&](int row) { const unsigned r = uid[row]; return r == TB_NONE ? -1ll : (long long)r; };

    // best and worst threshold of this lane's four rows; a row without thresholds has a worst one nothing comes before
    T best_s[4], worst_s[4];
    unsigned best_j[4], worst_j[4], n_r[4], all_r[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const unsigned n = gn[urow0 + r];
        n_r[r] = n;
        all_r[r] = 0;
        best_s[r] = Ts[(urow0 + r) * RB_GS];
        best_j[r] = Tj[(urow0 + r) * RB_GS];
        worst_s[r] = n > 0 ? Ts[(urow0 + r) * RB_GS + n - 1] : std::numeric_limits<T>::infinity();
        worst_j[r] = n > 0 ? Tj[(urow0 + r) * RB_GS + n - 1] : 0u;
    }

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, tb_all_items(a.dimB), [&](T (&acc)[4][4], unsigned j_base) {
        // ---- counting: the bins of rows 16 wave .. 16 wave + 15 are touched by this wave alone ----
#pragma unroll
        for (int r = 0; r < 4; r++) {
            bool some[4], any = false;   // comes before some threshold: before the worst one
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const unsigned j = j_base + 16 * t + col;
                some[t] = j < a.dimB && tb_better(acc[t][r], j, worst_s[r], worst_j[r]);
                any = any || some[t];
            }
            if (__ballot(any) == 0) continue;       // (uniform over the wave) every score of this pass died in registers
            bool mid[4], any_mid = false;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const bool all = some[t] && tb_better(acc[t][r], j_base + 16 * t + col, best_s[r], best_j[r]);   // before all of them
                all_r[r] += all ? 1u : 0u;
                mid[t] = some[t] && !all;
                any_mid = any_mid || mid[t];
            }
            if (__ballot(any_mid) == 0) continue;   // (uniform) the survivors counted in registers
            // before the worst threshold, not before the best: how many of thresholds 1 .. n - 2 it comes before besides.  The row's
            // thresholds are read once for the lane's four scores (the same address for the 16 lanes of a row: a broadcast); the
            // item indices are only looked at when some lane of the wave meets an equal score.
            const T* ts = Ts + (urow0 + r) * RB_GS;
            const unsigned* tj = Tj + (urow0 + r) * RB_GS;
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
                    for (int t = 0; t < 4; t++) beaten[t] += acc[t][r] == ti && j_base + 16 * t + col < ji ? 1u : 0u;
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (mid[t]) atomicAdd(&bins[(urow0 + r) * RB_GS + n - beaten[t]], 1u);   // (LDS, integer) the first threshold it comes before
        }
    });

    // ---- the slice's counts: a score before the best threshold is before every one of the group ----
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (all_r[r]) atomicAdd(&bins[(urow0 + r) * RB_GS], all_r[r]);
    __syncthreads();
    if (tid < TB_TU) {
        const unsigned n = gn[tid];
        unsigned run = 0;
        for (unsigned i = 0; i < n; i++) {
            run += bins[tid * RB_GS + i];
            if (run) atomicAdd(&a.dense[gs[tid] + i], run);   // (global, integer: the slices' counts add up in any order)
        }
    }
}

// one wave per chunk user
__global__ __launch_bounds__(256) void rank_excl_kernel(RbArgs a)
{
    const unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= a.n_users) return;   // (uniform over the wave)
    const unsigned p0 = a.tptr[i], nv = a.nvalid[i], u = a.arow[i];
    const real_t* ts = a.s_score + p0;
    const unsigned* tj = a.s_item + p0;
    unsigned n_excl = 0;
    auto subtract = [&](unsigned j) {
        if (nv == 0) return;
        const unsigned pos = rb_first_beaten(ts, tj, nv, rb_dot(a.A, a.B, a.k, u, j), j);
        if (pos < nv) atomicAdd(&a.corr[p0 + pos], 1u);
    };
    unsigned long long e0 = 0, e1 = 0;
    const TbExcl& x = a.excl;
    if (x.ex_indptr != nullptr) {
        e0 = x.ex_indptr[i];
        e1 = x.ex_indptr[i + 1];
        for (unsigned long long e = e0 + lane; e < e1; e += 64) subtract(x.ex_indices[e]);
        n_excl = (unsigned)(e1 - e0);
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
            if (mine) subtract(j);
            n_excl += (unsigned)__popcll(__ballot(mine));
        }
    }
    if (lane == 0) a.n_adm[i] = a.dimB - n_excl;
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct RbLayout {
    size_t chunk_users;      // users per chunk
    size_t cell_cap;         // held-out cells a chunk may carry
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t group_cap;
    size_t arow, tptr, ex_indptr, nvalid, n_adm, cell_row, cell_item, cell_score, cell_excl, s_score, s_item, s_origin, dense, corr, rank, grow,
        gstart, ex_indices, total;
    RbLayout(size_t n_users, size_t n_cells, size_t dimB)
    {
        const size_t R = sizeof(real_t), U = sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_cells = std::max<size_t>(n_cells, 1);
        dimB = std::max<size_t>(dimB, 1);
        const size_t uc = std::min(n_users, RB_CHUNK_USERS_MAX);
        idx_cap = std::min(RB_BUDGET / 2 / U, uc * dimB);   // (no overflow: 2^18 x 2^31)
        const size_t rest = RB_BUDGET - idx_cap * U - 32 * 20;   // (32: alignment of each of the parts)
        const size_t per_user = 5 * U + 2 * U + 2 * U;           // five per-user arrays (two of uc + 1), a group of its own
        const size_t per_cell = 8 * U + 2 * R + 1;               // eight index arrays, two of scores, 2 U / RB_G for the groups
        cell_cap = std::min((rest - per_user * uc - 64) / per_cell, n_cells);   // (>= RB_ROW_MAX whatever the arguments: see the static_assert)
        chunk_users = uc;
        group_cap = uc + cell_cap / RB_G + 1;
        TbTake take;
        arow = take(uc * U);
        tptr = take((uc + 1) * U);
        ex_indptr = take((uc + 1) * U);
        nvalid = take(uc * U);
        n_adm = take(uc * U);
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
        grow = take(group_cap * U);
        gstart = take(group_cap * U);
        ex_indices = take(idx_cap * U);
        total = take.o;
    }
};
// the least a chunk's cells get (every exclusion index and every user of a chunk present) holds the longest row a call accepts
static_assert((RB_BUDGET / 2 - 32 * 20 - 9 * sizeof(unsigned) * RB_CHUNK_USERS_MAX - 64) / (8 * sizeof(unsigned) + 2 * sizeof(real_t) + 1) >= RB_ROW_MAX,
              "one held-out row fits a chunk");

size_t rb_lds_bytes() { return 2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + (size_t)TB_TU * RB_GS * (sizeof(real_t) + 8) + (size_t)TB_TU * 12; }
// two workgroups per CU (160 KB of LDS), as topn_tile_kernel at its usual list sizes
static_assert(2 * (2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + (size_t)TB_TU * RB_GS * (sizeof(real_t) + 8) + (size_t)TB_TU * 12) <= 160 * 1024,
              "two workgroups of rank_tile_kernel per CU");

}  // namespace

extern "C" size_t poismf_hip_rank_batch_scratch_bytes(size_t n_users, size_t n_cells, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return RbLayout(n_users, n_cells, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_rank_batch_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                const sparse_ix* test_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || test_indptr == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (!tb_rows_ok(test_indptr, test_indices, n_users, dimB, RB_ROW_MAX)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, RbLayout(n_users, 1, dimB).idx_cap)) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_rank_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                              PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                              size_t* scratch_cap, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t n_cells = (size_t)test_indptr[n_users] - (size_t)test_indptr[0];
    const RbLayout L(n_users, n_cells, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;
    const size_t lds = rb_lds_bytes();
    auto kern = rank_tile_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    RbArgs a;
    std::vector<unsigned> hu, htp, hrow, hitem, hgrow, hgstart, hp, hx;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose held-out cells and exclusion lists fit their areas together
        size_t u1 = u0, nc = 0, nx = 0;
        while (u1 < n_users && u1 - u0 < L.chunk_users) {
            const size_t cells = (size_t)test_indptr[u1 + 1] - (size_t)test_indptr[u1];
            const size_t len = excl_indptr ? (size_t)excl_indptr[u1 + 1] - (size_t)excl_indptr[u1] : 0;
            if (u1 > u0 && (nc + cells > L.cell_cap || nx + len > L.idx_cap)) break;
            nc += cells;
            nx += len;
            u1++;
        }
        const size_t nu = u1 - u0;
        if (nc > L.cell_cap || nx > L.idx_cap) return 1;   // (cannot happen: the checks bound a single row by both)
        const size_t c_base = (size_t)test_indptr[u0];
        hu.resize(nu);
        htp.resize(nu + 1);
        hrow.resize(nc);
        hitem.resize(nc);
        hgrow.clear();
        hgstart.clear();
        for (size_t i = 0; i < nu; i++) {
            hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
            const size_t p0 = (size_t)test_indptr[u0 + i] - c_base, p1 = (size_t)test_indptr[u0 + i + 1] - c_base;
            htp[i] = (unsigned)p0;
            for (size_t p = p0; p < p1; p++) {
                hrow[p] = (unsigned)i;
                hitem[p] = (unsigned)test_indices[c_base + p];
            }
            for (size_t p = p0; p < p1; p += RB_G) {
                hgrow.push_back((unsigned)i);
                hgstart.push_back((unsigned)p);
            }
        }
        htp[nu] = (unsigned)nc;
        const size_t ng = hgrow.size();
        if (ng > L.group_cap) return 1;   // (cannot happen: a user adds at most one partial group)
        TB_TRY(pmf_upload(base + L.arow, hu.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.tptr, htp.data(), (nu + 1) * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_row, hrow.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_item, hitem.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.grow, hgrow.data(), ng * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.gstart, hgstart.data(), ng * sizeof(unsigned), stream));
        TB_TRY(tb_stage_excl(a.excl, seen, excl_indptr, excl_indices, u0, nu, nx, (unsigned*)(base + L.ex_indptr), (unsigned*)(base + L.ex_indices), hp,
                             hx, stream));
        TB_TRY(hipMemsetAsync(base + L.nvalid, 0, nu * sizeof(unsigned), stream));
        if (nc > 0) {
            TB_TRY(hipMemsetAsync(base + L.dense, 0, nc * sizeof(unsigned), stream));
            TB_TRY(hipMemsetAsync(base + L.corr, 0, nc * sizeof(unsigned), stream));
        }

        const size_t tiles = pmf_ceil_div(std::max<size_t>(ng, 1), TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, RB_TARGET_WGS);
        a.A = dA;
        a.B = dB;
        a.k = (int)k;
        a.dimB = (unsigned)dimB;
        a.n_users = (unsigned)nu;
        a.n_cells = (unsigned)nc;
        a.arow = (const unsigned*)(base + L.arow);
        a.tptr = (const unsigned*)(base + L.tptr);
        a.cell_row = (const unsigned*)(base + L.cell_row);
        a.cell_item = (const unsigned*)(base + L.cell_item);
        a.cell_score = (real_t*)(base + L.cell_score);
        a.cell_excl = (unsigned*)(base + L.cell_excl);
        a.s_score = (real_t*)(base + L.s_score);
        a.s_item = (unsigned*)(base + L.s_item);
        a.s_origin = (unsigned*)(base + L.s_origin);
        a.nvalid = (unsigned*)(base + L.nvalid);
        a.dense = (unsigned*)(base + L.dense);
        a.corr = (unsigned*)(base + L.corr);
        a.rank = (unsigned*)(base + L.rank);
        a.n_adm = (unsigned*)(base + L.n_adm);
        a.grow = (const unsigned*)(base + L.grow);
        a.gstart = (const unsigned*)(base + L.gstart);
        a.ngroups = (unsigned)ng;
        a.nslices = (unsigned)sl.nslices;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        a.iptr = nullptr;
        a.incl = nullptr;
        if (nc > 0) {
            const unsigned cell_blocks = (unsigned)pmf_ceil_div(nc, 256);
            hipLaunchKernelGGL(rank_threshold_kernel<false>, dim3(cell_blocks), dim3(256), 0, stream, a);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(rank_order_kernel, dim3(cell_blocks), dim3(256), 0, stream, a);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)sl.nslices), dim3(TB_WG), lds, stream, a);
            TB_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(rank_excl_kernel, dim3((unsigned)pmf_ceil_div(nu, 4)), dim3(256), 0, stream, a);
        TB_TRY(hipGetLastError());
        if (nc > 0) {
            hipLaunchKernelGGL(rank_finish_kernel<false>, dim3((unsigned)pmf_ceil_div(nu, 256)), dim3(256), 0, stream, a);
            TB_TRY(hipGetLastError());
            TB_TRY(pmf_download(out_rank + c_base, base + L.rank, nc * sizeof(unsigned), stream));
        }
        TB_TRY(pmf_download(out_n_adm + u0, base + L.n_adm, nu * sizeof(unsigned), stream));
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_rank_batch(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                          const sparse_ix* test_indptr, const sparse_ix* test_indices, const sparse_ix* excl_indptr,
                          const sparse_ix* excl_indices, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_batch_check(users, n_users, dimA, dimB, (size_t)k, test_indptr, test_indices, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_rank_batch_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, test_indptr, test_indices, nullptr,
                                                          excl_indptr, excl_indices, d_scratch, scratch_cap, out_rank, out_n_adm);
                     });
}

}  // extern "C"
