// rank_include.hip -- batched exact ranks among per-user candidate lists (include/poismf_hip.h, section 1j): for many users at once,
// the 0-based position of each held-out item among the user's OWN include list minus its exclusion set, under the total order "score
// descending, item index ascending".  Only the listed rows of B are read.  score(u, j) is section 1f's: the k-ordered fused chain,
// bit for bit what pair_dot_kernel (serve.hip) computes.
//
//   rank_threshold_kernel<true>  (tb_rank.hpp) a cell's score, and whether it leaves the ranking: in E(u), or not listed in I(u).
//   rank_order_kernel            (tb_rank.hpp) the user's valid thresholds best first.
//   rank_include_kernel          one wave per (user, slice of RI_SLICE candidates of its list), four waves per workgroup that share
//                                nothing -- no workgroup barrier, every LDS region belongs to one wave: the shape of
//                                topn_include_kernel, whose gather and chain (tb_gather.hpp) it uses.  The wave's LDS also holds the
//                                user's ordered thresholds (score, item) and one integer bin each, up to RI_G of them.  A candidate
//                                that is not in E(u) (tb_excluded) adds 1 to the wave's admissible count and, by a binary search
//                                over the ordered thresholds, 1 to the bin of the first threshold it comes before (LDS integer
//                                add), if there is one.  The held-out item itself is a candidate with the bits of its own threshold
//                                and never comes before itself.  At the end the running sums over the bins are the slice's counts;
//                                they go to the cells' global counters, the admissible count to N(u), with integer atomics: the
//                                slices of one user run in different waves and their order cannot matter.  A user with more than
//                                RI_G valid held-out items keeps nothing in LDS: its candidates search the ordered thresholds in
//                                global memory and add 1 to the global difference array, which rank_finish_kernel sums.  A user
//                                without a valid held-out item is not gathered at all: only N(u) is counted.
//   rank_finish_kernel<true>     (tb_rank.hpp) rank = counter + running sum of the difference array, in the caller's order.
//
// Excluded candidates are dropped before they are counted, so section 1g's correction pass has no counterpart.  All counting is in
// integers; no float atomics.  A list is cut by the one fixed slice length: nothing is merged, so nothing grows it.  The host side cuts
// the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a chunk (RiLayout;
// poismf_hip_rank_include_scratch_bytes reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_rank.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int RI_WAVES = 4;                               // work items per workgroup
constexpr unsigned RI_G = POISMF_HIP_RANK_INCLUDE_GROUP;  // thresholds (and bins) a wave keeps in LDS
constexpr size_t RI_SLICE = POISMF_HIP_RANK_INCLUDE_SLICE;   // candidates per work item
constexpr size_t RI_MAX_ROW = POISMF_HIP_TOPN_INCLUDE_MAX_ROW;
static_assert(RI_G == 128, "the running sums of a wave: two bins per lane");
static_assert(RI_SLICE % 64 == 0, "a slice is whole passes of 64 candidates");
static_assert(RI_MAX_ROW * sizeof(unsigned) == TB_BUDGET / 4, "the longest include row fills a quarter of the scratch");
static_assert(POISMF_HIP_RANK_BATCH_BUDGET_MB == POISMF_HIP_TOPN_BATCH_BUDGET_MB, "one budget for the calls that share a session's scratch");

struct RiItem { unsigned ui, p0, len; };                  // chunk user, first candidate in the chunk's index area, candidates

struct RiArgs {
    RbArgs r;
    const RiItem* items;
    unsigned n_items;
};

__host__ __device__ constexpr size_t ri_wave_lds(size_t k)
{
    return (64 * (size_t)TI_SLOT + ((k + 3) & ~(size_t)3) * TI_R + RI_G * (TI_R + 2 * sizeof(unsigned)) + 15) & ~(size_t)15;
}
// two workgroups per CU (160 KB of LDS) at k = 50, as topn_include_kernel
static_assert(2 * RI_WAVES * ri_wave_lds(50) <= 160 * 1024, "two workgroups of rank_include_kernel per CU at k = 50");

__global__ __launch_bounds__(64 * RI_WAVES) void rank_include_kernel(RiArgs a)
{
    extern __shared__ __align__(16) unsigned char ri_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned item = blockIdx.x * RI_WAVES + wave;
    if (item >= a.n_items) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.r.k;
    const int ka = (k + 3) & ~3;
    unsigned char* Bs = ri_smem + wave * ri_wave_lds((size_t)k);   // [64][TI_SLOT]: the pass's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                     // [ka] the user's row, zero padded
    real_t* Ts = As + ka;                                          // [RI_G] the user's thresholds, best first: score ...
    unsigned* Tj = (unsigned*)(Ts + RI_G);                         // ... and item
    unsigned* bins = Tj + RI_G;                                    // [RI_G] candidates whose first beaten threshold is this one

    const RiItem it = a.items[item];
    const unsigned arow = a.r.arow[it.ui];
    const unsigned t0 = a.r.tptr[it.ui], nv = a.r.nvalid[it.ui];
    const bool big = nv > RI_G;             // (uniform) the thresholds stay in global memory
    const unsigned n = big ? 0u : nv;       // thresholds in LDS
    const unsigned* lst = a.r.incl + it.p0;
    unsigned adm = 0;                       // (uniform) candidates of the slice that are not in E(u)

    if (nv == 0) {   // nothing to rank: N(u) alone, no row of B is read
        for (unsigned e0 = 0; e0 < it.len; e0 += 64) {
            const bool ok = e0 + lane < it.len && !tb_excluded(a.r.excl, it.ui, arow, lst[e0 + lane]);
            adm += (unsigned)__popcll(__ballot(ok));
        }
        if (lane == 0 && adm) atomicAdd(&a.r.n_adm[it.ui], adm);
        return;
    }

    const real_t* Au = a.r.A + (size_t)arow * (size_t)k;
    for (int c = (int)lane; c < ka; c += 64) As[c] = c < k ? Au[c] : (real_t)0;
    for (unsigned i = lane; i < RI_G; i += 64) {
        Ts[i] = i < n ? a.r.s_score[t0 + i] : (real_t)0;
        Tj[i] = i < n ? a.r.s_item[t0 + i] : 0u;
        bins[i] = 0;
    }
    tb_wave_sync();

    const unsigned npass = (it.len + 63) / 64;
    const TiGather g = { (const char*)a.r.B, Bs, k, lane >> 2, lane & 3 };
    ti_u32x4 pre[TI_NI];
    unsigned j_cur = lane < it.len ? lst[lane] : TB_NONE;
    unsigned j_nxt = 64 + lane < it.len ? lst[64 + lane] : TB_NONE;
    if (npass) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);

    for (unsigned pass = 0; pass < npass; pass++) {
        const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, pass, npass);
        // ---- counting ----
        const bool ok = j_cur != TB_NONE && !tb_excluded(a.r.excl, it.ui, arow, j_cur);
        adm += (unsigned)__popcll(__ballot(ok));
        if (ok) {
            if (big) {
                const unsigned pos = rb_first_beaten(a.r.s_score + t0, a.r.s_item + t0, nv, s, j_cur);
                if (pos < nv) atomicAdd(&a.r.corr[t0 + pos], 1u);   // (global, integer)
            } else {
                const unsigned pos = rb_first_beaten(Ts, Tj, n, s, j_cur);
                if (pos < n) atomicAdd(&bins[pos], 1u);             // (LDS, integer)
            }
        }
        j_cur = j_nxt;
        const unsigned nx = (pass + 2) * 64 + lane;
        j_nxt = nx < it.len ? lst[nx] : TB_NONE;
    }

    // ---- the slice's counts: a candidate before threshold i is before every later one ----
    tb_wave_sync();
    if (!big) {
        unsigned run0 = 0, run1 = 0;   // of thresholds lane and 64 + lane
        for (unsigned q = 0; q < n; q++) {
            const unsigned b = bins[q];   // (one address for the wave: a broadcast)
            run0 += q <= lane ? b : 0u;
            run1 += q <= 64 + lane ? b : 0u;
        }
        if (lane < n && run0) atomicAdd(&a.r.dense[t0 + lane], run0);             // (global, integer: the slices' counts add up in any order)
        if (64 + lane < n && run1) atomicAdd(&a.r.dense[t0 + 64 + lane], run1);
    }
    if (lane == 0 && adm) atomicAdd(&a.r.n_adm[it.ui], adm);
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct RiLayout {
    size_t chunk_users;      // users per chunk
    size_t cell_cap;         // held-out cells a chunk may carry
    size_t incl_cap;         // include indices a chunk may carry
    size_t excl_cap;         // exclusion indices a chunk may carry
    size_t item_cap;         // work items of a chunk
    size_t arow, tptr, iptr, ex_indptr, nvalid, n_adm, cell_row, cell_item, cell_score, cell_excl, s_score, s_item, s_origin, dense, corr, rank,
        items, incl, ex_indices, total;
    RiLayout(size_t n_users, size_t n_test, size_t n_incl, size_t dimB)
    {
        const size_t R = sizeof(real_t), U = sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_test = std::max<size_t>(n_test, 1);
        dimB = std::max<size_t>(dimB, 1);
        chunk_users = std::min(n_users, TB_CHUNK_USERS_MAX);
        incl_cap = std::min(RI_MAX_ROW, std::max<size_t>(n_incl, 1));                       // a quarter of the budget at most
        excl_cap = std::min(TB_BUDGET / 2 / U, chunk_users * dimB);                         // section 1f's: half of it  (no overflow: 2^18 x 2^31)
        item_cap = chunk_users + incl_cap / RI_SLICE;                                       // a list of len candidates has at most len / RI_SLICE + 1 slices
        const size_t rest = TB_BUDGET - (incl_cap + excl_cap) * U - 32 * 20;                // (32: alignment of each of the parts)
        const size_t per_user = 6 * U + 3 * U;                                              // six per-user arrays (three of chunk_users + 1)
        const size_t per_cell = 8 * U + 2 * R;                                              // eight index arrays, two of scores
        cell_cap = std::min((rest - per_user * chunk_users - item_cap * sizeof(RiItem)) / per_cell, n_test);   // (>= RB_ROW_MAX: see the static_assert)
        TbTake take;
        arow = take(chunk_users * U);
        tptr = take((chunk_users + 1) * U);
        iptr = take((chunk_users + 1) * U);
        ex_indptr = take((chunk_users + 1) * U);
        nvalid = take(chunk_users * U);
        n_adm = take(chunk_users * U);
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
        items = take(item_cap * sizeof(RiItem));
        incl = take(incl_cap * U);
        ex_indices = take(excl_cap * U);
        total = take.o;
    }
};
// the least a chunk's cells get (every include and exclusion index, every user and every work item of a chunk present) holds the longest
// held-out row a call accepts
static_assert((TB_BUDGET / 4 - 32 * 20 - 9 * sizeof(unsigned) * TB_CHUNK_USERS_MAX - (TB_CHUNK_USERS_MAX + RI_MAX_ROW / RI_SLICE) * sizeof(RiItem)) /
                      (8 * sizeof(unsigned) + 2 * sizeof(real_t)) >= RB_ROW_MAX,
              "one held-out row fits a chunk");

}  // namespace

extern "C" size_t poismf_hip_rank_include_scratch_bytes(size_t n_users, size_t n_test_cells, size_t n_incl_cells, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return RiLayout(n_users, n_test_cells, n_incl_cells, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_rank_include_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                  const sparse_ix* test_indices, const sparse_ix* incl_indptr, const sparse_ix* incl_indices,
                                  const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || test_indptr == nullptr || incl_indptr == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (!tb_rows_ok(test_indptr, test_indices, n_users, dimB, RB_ROW_MAX)) return 2;
    if (!tb_rows_ok(incl_indptr, incl_indices, n_users, dimB, RI_MAX_ROW)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_rank_include_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                                const sparse_ix* incl_indptr, const sparse_ix* incl_indices, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, unsigned int* out_rank,
                                unsigned int* out_n_adm)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t n_test = (size_t)test_indptr[n_users] - (size_t)test_indptr[0];
    const size_t n_incl = (size_t)incl_indptr[n_users] - (size_t)incl_indptr[0];
    const RiLayout L(n_users, n_test, n_incl, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;
    const size_t lds = RI_WAVES * ri_wave_lds(k);
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rank_include_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(RI_WAVES * ri_wave_lds(TB_K_MAX))));

    RiArgs a;
    RbArgs& r = a.r;
    std::vector<unsigned> hu, htp, hq, hrow, hitem, hi, hp, hx;
    std::vector<RiItem> items;
    auto row_len = [](const sparse_ix* indptr, size_t i) { return indptr ? (size_t)indptr[i + 1] - (size_t)indptr[i] : 0; };
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose held-out cells, include lists and exclusion lists fit their areas together
        size_t u1 = u0, nc = 0, ni = 0, nx = 0;
        while (u1 < n_users && u1 - u0 < L.chunk_users) {
            const size_t cells = row_len(test_indptr, u1), len_i = row_len(incl_indptr, u1), len_e = row_len(excl_indptr, u1);
            if (u1 > u0 && (nc + cells > L.cell_cap || ni + len_i > L.incl_cap || nx + len_e > L.excl_cap)) break;
            nc += cells;
            ni += len_i;
            nx += len_e;
            u1++;
        }
        const size_t nu = u1 - u0;
        if (nc > L.cell_cap || ni > L.incl_cap || nx > L.excl_cap) return 1;   // (cannot happen: the checks bound a single row by all three)
        const size_t c_base = (size_t)test_indptr[u0], i_base = (size_t)incl_indptr[u0];
        hu.resize(nu);
        htp.resize(nu + 1);
        hq.resize(nu + 1);
        hrow.resize(nc);
        hitem.resize(nc);
        hi.resize(ni);
        items.clear();
        for (size_t i = 0; i < nu; i++) {
            hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
            const size_t p0 = (size_t)test_indptr[u0 + i] - c_base, p1 = (size_t)test_indptr[u0 + i + 1] - c_base;
            htp[i] = (unsigned)p0;
            for (size_t p = p0; p < p1; p++) {
                hrow[p] = (unsigned)i;
                hitem[p] = (unsigned)test_indices[c_base + p];
            }
            // the plan: one work item per (user, slice); an empty list has none and keeps N(u) = 0
            const size_t q0 = (size_t)incl_indptr[u0 + i] - i_base, len = row_len(incl_indptr, u0 + i);
            hq[i] = (unsigned)q0;
            for (size_t s = 0; s < len; s += RI_SLICE) items.push_back({ (unsigned)i, (unsigned)(q0 + s), (unsigned)std::min(RI_SLICE, len - s) });
        }
        htp[nu] = (unsigned)nc;
        hq[nu] = (unsigned)ni;
        for (size_t p = 0; p < ni; p++) hi[p] = (unsigned)incl_indices[i_base + p];
        if (items.size() > L.item_cap) return 1;   // (cannot happen: a user adds at most one partial slice)
        TB_TRY(pmf_upload(base + L.arow, hu.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.tptr, htp.data(), (nu + 1) * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.iptr, hq.data(), (nu + 1) * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_row, hrow.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.cell_item, hitem.data(), nc * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.incl, hi.data(), ni * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.items, items.data(), items.size() * sizeof(RiItem), stream));
        TB_TRY(tb_stage_excl(r.excl, seen, excl_indptr, excl_indices, u0, nu, nx, (unsigned*)(base + L.ex_indptr), (unsigned*)(base + L.ex_indices), hp,
                             hx, stream));
        TB_TRY(hipMemsetAsync(base + L.nvalid, 0, nu * sizeof(unsigned), stream));
        TB_TRY(hipMemsetAsync(base + L.n_adm, 0, nu * sizeof(unsigned), stream));
        if (nc > 0) {
            TB_TRY(hipMemsetAsync(base + L.dense, 0, nc * sizeof(unsigned), stream));
            TB_TRY(hipMemsetAsync(base + L.corr, 0, nc * sizeof(unsigned), stream));
        }
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
        r.grow = nullptr;
        r.gstart = nullptr;
        r.ngroups = r.nslices = r.tiles_per_slice = 0;
        r.iptr = (const unsigned*)(base + L.iptr);
        r.incl = (const unsigned*)(base + L.incl);
        a.items = (const RiItem*)(base + L.items);
        a.n_items = (unsigned)items.size();
        if (nc > 0) {
            const unsigned cell_blocks = (unsigned)pmf_ceil_div(nc, 256);
            hipLaunchKernelGGL(rank_threshold_kernel<true>, dim3(cell_blocks), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
            hipLaunchKernelGGL(rank_order_kernel, dim3(cell_blocks), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
        }
        if (!items.empty()) {
            hipLaunchKernelGGL(rank_include_kernel, dim3((unsigned)pmf_ceil_div(items.size(), RI_WAVES)), dim3(64 * RI_WAVES), lds, stream, a);
            TB_TRY(hipGetLastError());
        }
        if (nc > 0) {
            hipLaunchKernelGGL(rank_finish_kernel<true>, dim3((unsigned)pmf_ceil_div(nu, 256)), dim3(256), 0, stream, r);
            TB_TRY(hipGetLastError());
            TB_TRY(pmf_download(out_rank + c_base, base + L.rank, nc * sizeof(unsigned), stream));
        }
        TB_TRY(pmf_download(out_n_adm + u0, base + L.n_adm, nu * sizeof(unsigned), stream));
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_rank_include(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            const sparse_ix* test_indptr, const sparse_ix* test_indices, const sparse_ix* incl_indptr,
                            const sparse_ix* incl_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, unsigned int* out_rank,
                            unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_include_check(users, n_users, dimA, dimB, (size_t)k, test_indptr, test_indices, incl_indptr, incl_indices,
                                                     excl_indptr, excl_indices))
        return rc;
    // (tb_dropin's copy of B carries the 16 bytes of slack the gather may read past a row)
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_rank_include_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, test_indptr, test_indices,
                                                            incl_indptr, incl_indices, nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap,
                                                            out_rank, out_n_adm);
                     });
}

}  // extern "C"
