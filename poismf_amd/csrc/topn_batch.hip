// topn_batch.hip -- batched top-N (include/poismf_hip.h, section 1f): for many users at once, the n_top best items of each under
// the total order "score descending, item index ascending", minus per-user exclusion sets.
//
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t
//
// which is bit for bit what pair_dot_kernel (serve.hip: predict_multiple, poismf_hip_session_predict) computes.  It is NOT
// score_kernel's order (sixteen strided partial chains and a butterfly), so the last bit may differ from topN's score.
//
// One kernel (topn_tile_kernel): a workgroup of four waves owns a tile of TB_TU = 64 users (wave w: users 16 w .. 16 w + 15) and a
// slice of the items, which it walks TB_TJ = 64 items at a time.  The users' rows and the items' rows go through LDS in chunks of
// TB_KC columns, zero padded to a multiple of four columns (fma(0, 0, s) = s for every s such a chain can hold: it starts at +0 and is
// never -0).  fp32: v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain from C = 0; four independent accumulators
// (16 users x 64 items) per wave.  fp64: a VALU fma chain with the same register layout (one accumulator per (user, item), k
// ascending) -- whether v_mfma_f64_16x16x4_f64 rounds as that chain does has not been measured, so it is not used.
// Scores die in registers unless they beat the user's threshold (the n_top-th best so far, kept in LDS with its item index);
// a survivor is then looked up in the exclusion lists (binary search; linear scan of a resident row not known to be sorted) and
// appended to the user's candidate list in LDS: the selection of tb_select.hpp (TbSelect), which topn_quota.hip and topn_shared.hip
// drive too.  Per (user, slice) the sorted best n_top go to scratch; topn_merge_kernel ranks the slices' lists of a user the same way.
// No float atomics anywhere.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a
// chunk's user list, exclusion lists, partial lists and results (TbLayout; poismf_hip_topn_batch_scratch_bytes reports its size).
#include <cstring>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"

namespace {

constexpr size_t TB_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many
static_assert(TB_N_TOP_MAX >= 128, "the header promises at least 128");
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, 0) <= TB_LDS_LIMIT, "the two tiles and 64 lists of the deepest n_top with TB_ROOM free slots fit LDS");

struct TbArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users
    real_t* part_score;               // [n_users][nslices][n_top]
    unsigned* part_ix;
};

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void topn_tile_kernel(TbArgs a)
{
    extern __shared__ __align__(16) unsigned char tb_smem[];
    T* As = (T*)tb_smem;                                  // [TB_TU][TB_KS]
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
    sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);
}

// (topn_merge_kernel, one wave per user over its nslices sorted partial lists, lives in tb_select.hpp: topn_weighted.hip launches it too)

// exclude_seen needs to know whether the resident rows may be binary-searched: flag[0] = 1 when some row is not strictly ascending
__global__ __launch_bounds__(256) void topn_rows_sorted_kernel(const unsigned long long* indptr, const unsigned* indices, size_t nrows, unsigned* flag)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long p1 = indptr[r + 1];
        for (unsigned long long p = indptr[r] + 1; p < p1; p++)
            if (indices[p - 1] >= indices[p]) { flag[0] = 1u; break; }
    }
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct TbLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t part_entries;     // (user, slice, rank) entries of the partial lists
    size_t users, ex_indptr, ex_indices, part_score, part_ix, out_score, out_ix, total;
    TbLayout(size_t n_users, size_t n_top, size_t dimB)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::max<size_t>(dimB, 1);
        const size_t first = std::min(n_users, TB_CHUNK_USERS_MAX);
        idx_cap = std::min(TB_BUDGET / 2 / sizeof(unsigned), first * dimB);   // (no overflow: 2^18 x 2^31)
        const size_t rest = TB_BUDGET - idx_cap * sizeof(unsigned) - 256;     // (256: alignment of the seven parts)
        // partial lists: users x slices <= TB_TU x (TB_TARGET_WGS + tiles)  (tb_slices), results: users
        const size_t fixed = 16 + (TB_TU * TB_TARGET_WGS + TB_TU) * n_top * (R + 4);
        const size_t per_user = 8 + 2 * n_top * (R + 4);
        size_t uc = (rest - fixed) / per_user;
        uc = std::min(std::min(uc, TB_CHUNK_USERS_MAX), n_users);
        if (uc > TB_TU) uc -= uc % TB_TU;
        chunk_users = uc;
        part_entries = (TB_TU * TB_TARGET_WGS + TB_TU + uc) * n_top;   // (every chunk of <= uc users fits, however it is sliced)
        TbTake take;
        users = take(uc * sizeof(unsigned));
        ex_indptr = take((uc + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        part_score = take(part_entries * R);
        part_ix = take(part_entries * sizeof(unsigned));
        out_score = take(uc * n_top * R);
        out_ix = take(uc * n_top * sizeof(unsigned));
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_batch_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TbLayout(n_users, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_batch_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX || n_top > dimB) return 2;
    if (k < 1 || k > TB_K_MAX || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (excl_indptr != nullptr) {
        if (!tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TbLayout(n_users, n_top, dimB).idx_cap)) return 2;
        for (size_t i = 0; i < n_users; i++)
            if (n_top > dimB - ((size_t)excl_indptr[i + 1] - (size_t)excl_indptr[i])) return 2;   // n_top items must remain
    }
    return 0;
}

// exclude_seen: finds out, once per session, whether the resident rows are strictly ascending (*seen.sorted); 0, or 1 on a device error
int poismf_hip_topn_seen_sorted(PmfTopnSeen& seen, hipStream_t stream)
{
    if (*seen.sorted >= 0) return 0;
    const size_t nrows = seen.row_end - seen.row_begin;
    unsigned* d_flag = nullptr;
    unsigned flag = 0;
    TB_TRY(pmf_alloc(&d_flag, sizeof(unsigned), stream));
    hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(unsigned), stream);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<size_t>(pmf_ceil_div(std::max<size_t>(nrows, 1), 256), 4096);
        hipLaunchKernelGGL(topn_rows_sorted_kernel, dim3(grid), dim3(256), 0, stream, seen.d_indptr, seen.d_indices, nrows, d_flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = pmf_download(&flag, d_flag, sizeof(unsigned), stream);
    pmf_free(d_flag, stream);
    TB_TRY(e);
    *seen.sorted = flag ? 0 : 1;
    return 0;
}

// exclude_seen (after poismf_hip_topn_batch_check): the shard must hold every user, and every user must keep n_top admissible items.
// Row lengths come from a host copy of the row pointers (fetched once per session); only a user whose two lists together could
// leave fewer than n_top items has its resident row fetched and the union counted.  0, 1 (device error) or 2.
static int tb_check_seen(PmfTopnSeen& seen, const sparse_ix* users, size_t n_users, size_t n_top, size_t dimB, const sparse_ix* excl_indptr,
                         const sparse_ix* excl_indices, hipStream_t stream)
{
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] < seen.row_begin || (size_t)users[i] >= seen.row_end) return 2;
    const size_t nrows = seen.row_end - seen.row_begin;
    std::vector<unsigned long long>& ip = *seen.h_indptr;
    if (ip.size() != nrows + 1) {
        ip.resize(nrows + 1);
        TB_TRY(pmf_download(ip.data(), seen.d_indptr, (nrows + 1) * sizeof(unsigned long long), stream));
    }
    if (poismf_hip_topn_seen_sorted(seen, stream)) return 1;
    std::vector<unsigned> row;
    for (size_t i = 0; i < n_users; i++) {
        const size_t r = (size_t)users[i] - seen.row_begin;
        const size_t len_s = (size_t)(ip[r + 1] - ip[r]);
        const size_t len_e = excl_indptr ? (size_t)excl_indptr[i + 1] - (size_t)excl_indptr[i] : 0;
        if (len_s + len_e <= dimB - n_top) continue;
        row.resize(len_s);
        TB_TRY(pmf_download(row.data(), seen.d_indices + ip[r], len_s * sizeof(unsigned), stream));
        for (size_t p = 0; p < len_e; p++) row.push_back((unsigned)excl_indices[(size_t)excl_indptr[i] + p]);
        std::sort(row.begin(), row.end());
        const size_t uniq = (size_t)(std::unique(row.begin(), row.end()) - row.begin());
        if (uniq > dimB - n_top) return 2;
    }
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                              const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr)
        if (const int rc = tb_check_seen(*seen, users, n_users, n_top, dimB, excl_indptr, excl_indices, stream)) return rc;
    const TbLayout L(n_users, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, 0);
    const size_t lds = tb_lds_bytes(cap, 0);
    auto kern = topn_tile_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));

    TbArgs a;
    std::vector<unsigned> hu, hp, hx, hix;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose exclusion lists fit the index area together
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, TB_TARGET_WGS, std::max<size_t>(1, TB_MERGE_MAX / n_top));   // (the merge kernel's LDS bounds them)
        const size_t nslices = sl.nslices;
        if (nu * nslices * n_top > L.part_entries) return 1;   // (cannot happen: TbLayout sizes the lists for any slicing of a chunk)
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
        // (one slice: its sorted lists are the results)
        a.part_score = (real_t*)(base + (nslices == 1 ? L.out_score : L.part_score));
        a.part_ix = (unsigned*)(base + (nslices == 1 ? L.out_ix : L.part_ix));
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            hipLaunchKernelGGL(topn_merge_kernel<false>, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, (unsigned)nu, (unsigned)nslices,
                               (unsigned)n_top, (real_t*)(base + L.out_score), (unsigned*)(base + L.out_ix));
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score), hix, out_ix, out_score, stream)) return 1;
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_batch(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                          size_t n_top, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_batch_check(users, n_users, n_top, dimA, dimB, (size_t)k, excl_indptr, excl_indices)) return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_batch_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, nullptr, excl_indptr,
                                                          excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
