// tb_batch.hpp -- the host side the batched top-N (topn_batch.hip, topn_include.hip, topn_shared.hip, topn_deep.hip, topn_quota.hip, topn_weighted.hip,
// topn_diverse.hip, topn_adjust.hip) and
// the batched ranks (rank_batch.hip, rank_include.hip, rank_shared.hip) have in common -- the top-N cores' chunk loop opens with
// tb_stage_chunk and closes with tb_fetch_results -- and what the session (session.hip) hands to their cores
#pragma once
#include <cstddef>
#include <cstring>
#include <algorithm>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"

// exclude_seen: the session's resident CSR shard, and what the session remembers about it between calls
struct PmfTopnSeen {
    const unsigned long long* d_indptr;          // [row_end - row_begin + 1], from 0
    const unsigned* d_indices;
    size_t row_begin, row_end;                   // the shard's rows of A
    std::vector<unsigned long long>* h_indptr;   // host copy of d_indptr (empty until the first call needs it)
    int* sorted;                                 // -1 not checked yet, 0 some row is not strictly ascending, 1 all are
};

// (topn_batch.hip) finds out, once per session, whether the resident rows are strictly ascending (*seen.sorted); 0, or 1 on a device error
int poismf_hip_topn_seen_sorted(PmfTopnSeen& seen, hipStream_t stream);

// The argument checks of an entry point: 0, or 2.  No device call.
int poismf_hip_topn_batch_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_rank_batch_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                const sparse_ix* test_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices);

// The cores on device-resident factors (the session and the drop-in).  Arguments already checked.  dA rows are addressed by users[i], or
// by i itself when compact_A (the drop-in uploads only the batch's rows).  *d_scratch / *scratch_cap: the caller's scratch, grown when it
// is smaller than the call needs.  Return 0, 1 or (top-N with exclude_seen) 2.
int poismf_hip_topn_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                              const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);
int poismf_hip_rank_batch_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                              PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                              size_t* scratch_cap, unsigned int* out_rank, unsigned int* out_n_adm);

// (topn_include.hip; section 1h) the same pair for the top-N over include lists: the check makes no device call, the core returns 0 or 1
int poismf_hip_topn_include_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                  const sparse_ix* incl_indptr, const sparse_ix* incl_indices, const sparse_ix* excl_indptr,
                                  const sparse_ix* excl_indices);
int poismf_hip_topn_include_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* incl_indptr,
                                const sparse_ix* incl_indices, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);

// (topn_shared.hip; section 1i) the same pair for the top-N over lists shared between users: list_of[i] names user i's row of the table
int poismf_hip_topn_shared_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                 const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of,
                                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_topn_shared_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                               const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* list_indptr,
                               const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of, PmfTopnSeen* seen,
                               const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap,
                               sparse_ix* out_ix, real_t* out_score);

// (rank_include.hip; section 1j) the same pair for the ranks among per-user include lists: the check makes no device call, the core
// returns 0 or 1
int poismf_hip_rank_include_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                  const sparse_ix* test_indices, const sparse_ix* incl_indptr, const sparse_ix* incl_indices,
                                  const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_rank_include_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                                const sparse_ix* incl_indptr, const sparse_ix* incl_indices, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, unsigned int* out_rank,
                                unsigned int* out_n_adm);

// (rank_shared.hip; section 1k) the same pair for the ranks among lists shared between users: list_of[i] names user i's row of the table
int poismf_hip_rank_shared_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* test_indptr,
                                 const sparse_ix* test_indices, const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists,
                                 const sparse_ix* list_of, const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_rank_shared_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                               const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr, const sparse_ix* test_indices,
                               const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of,
                               bool unite_test, PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                               void** d_scratch, size_t* scratch_cap, unsigned int* out_rank, unsigned int* out_n_adm);

// (topn_quota.hip; section 1n) the same pair for the top-N with per-group quotas: group_of [dimB] and quota [n_groups] are host arrays;
// the check makes no device call, the core returns 0 or 1
int poismf_hip_topn_quota_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                const sparse_ix* group_of, size_t n_groups, const sparse_ix* quota, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices);
int poismf_hip_topn_quota_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                              const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* group_of, size_t n_groups,
                              const sparse_ix* quota, PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                              void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);

// (topn_weighted.hip; section 1o) the same pair for the top-N with per-item score weights: item_weight [dimB] is a host array; the
// check makes no device call, the core returns 0 or 1.  The core reads dA and dB only: the session passes its B for both when the
// queries are rows of B
int poismf_hip_topn_weighted_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                   const real_t* item_weight, const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_topn_weighted_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                 const sparse_ix* users, size_t n_users, size_t n_top, const real_t* item_weight, PmfTopnSeen* seen,
                                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap,
                                 sparse_ix* out_ix, real_t* out_score);

// (topn_adjust.hip; section 1r) the same pair for the top-N with per-(user, item) score factors: the adjust list is a host CSR with
// one row per user of the batch and real_t factors; the check makes no device call, the core returns 0 or 1
int poismf_hip_topn_adjusted_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                   const sparse_ix* adj_indptr, const sparse_ix* adj_indices, const real_t* adj_factor,
                                   const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_topn_adjusted_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                 const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* adj_indptr,
                                 const sparse_ix* adj_indices, const real_t* adj_factor, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                 const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);

// (topn_diverse.hip; section 1p) the same pair for the diversified top-N: greedy MMR over the best `pool` items; item_inv_norm [dimB] is
// a host array; the check makes no device call, the core returns 0 or 1.  out_score and out_value may be NULL
int poismf_hip_topn_diverse_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t pool, double lambda, size_t dimA, size_t dimB,
                                  size_t k, const real_t* item_inv_norm, const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
int poismf_hip_topn_diverse_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, size_t pool, double lambda, const real_t* item_inv_norm,
                                PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                                size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score, real_t* out_value);

#define TB_TRY(expr) do { if ((expr) != hipSuccess) return 1; } while (0)

namespace {

constexpr size_t TB_K_MAX = sizeof(real_t) == 4 ? 512 : 256;   // what a session supports
constexpr size_t TB_CHUNK_USERS_MAX = 262144;
constexpr size_t TB_N_TOP_MAX = POISMF_HIP_TOPN_BATCH_MAX_N_TOP;
constexpr size_t TB_BUDGET = (size_t)POISMF_HIP_TOPN_BATCH_BUDGET_MB << 20;

// the parts of a scratch layout, one after the other: take(bytes) is where the next part starts; `o` ends as the total
struct TbTake {
    size_t o = 0;
    size_t operator()(size_t bytes) { const size_t at = o; o = pmf_round_up(o + bytes, 32); return at; }
};

// A CSR-shaped list with one row per user: row pointers from a non-negative start that never decrease, no row longer than row_max (or
// dimB), indices below dimB and strictly ascending within a row.
inline bool tb_rows_ok(const sparse_ix* indptr, const sparse_ix* indices, size_t n_users, size_t dimB, size_t row_max)
{
    if ((long long)indptr[0] < 0) return false;
    for (size_t i = 0; i < n_users; i++) {
        if (indptr[i + 1] < indptr[i]) return false;
        const size_t p0 = (size_t)indptr[i], p1 = (size_t)indptr[i + 1];
        if (p1 - p0 > dimB || p1 - p0 > row_max) return false;
        if (p1 > p0 && indices == nullptr) return false;
        for (size_t p = p0; p < p1; p++) {
            if ((long long)indices[p] < 0 || (size_t)indices[p] >= dimB) return false;
            if (p > p0 && (size_t)indices[p - 1] >= (size_t)indices[p]) return false;
        }
    }
    return true;
}

// The items cut into slices for `row_tiles` tiles of users: about target_wgs workgroups in all, at most `cap` slices.
struct TbSlices { size_t tiles_per_slice, nslices; };
inline TbSlices tb_slices(size_t row_tiles, size_t dimB, size_t target_wgs, size_t cap = (size_t)-1)
{
    const size_t item_tiles = pmf_ceil_div(dimB, TB_TJ);
    const size_t want = std::max<size_t>(std::min({ row_tiles >= target_wgs ? 1 : pmf_ceil_div(target_wgs, row_tiles), item_tiles, cap }), 1);
    const size_t tps = pmf_ceil_div(item_tiles, want);
    return { tps, pmf_ceil_div(item_tiles, tps) };
}

// The exclusion test of a chunk of users u0 .. u0 + nu - 1 whose lists hold nx indices: the lists go to d_indptr / d_indices rebased to
// the chunk (hp, hx: staging the caller keeps between chunks), the resident rows are `seen`'s.
inline hipError_t tb_stage_excl(TbExcl& x, const PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, size_t u0,
                                size_t nu, size_t nx, unsigned* d_indptr, unsigned* d_indices, std::vector<unsigned>& hp,
                                std::vector<unsigned>& hx, hipStream_t stream)
{
    x.seen_indptr = seen ? seen->d_indptr : nullptr;
    x.seen_indices = seen ? seen->d_indices : nullptr;
    x.seen_row0 = seen ? (unsigned)seen->row_begin : 0u;
    x.seen_sorted = seen ? *seen->sorted : 0;
    x.ex_indptr = excl_indptr ? d_indptr : nullptr;
    x.ex_indices = d_indices;
    if (excl_indptr == nullptr) return hipSuccess;
    hp.resize(nu + 1);
    hx.resize(nx);
    const size_t p_base = (size_t)excl_indptr[u0];
    for (size_t i = 0; i <= nu; i++) hp[i] = (unsigned)((size_t)excl_indptr[u0 + i] - p_base);
    for (size_t p = 0; p < nx; p++) hx[p] = (unsigned)excl_indices[p_base + p];
    const hipError_t e = pmf_upload(d_indptr, hp.data(), (nu + 1) * sizeof(unsigned), stream);
    return e != hipSuccess ? e : pmf_upload(d_indices, hx.data(), nx * sizeof(unsigned), stream);
}

// ---- the chunk loop of the six top-N cores (topn_batch.hip, topn_include.hip, topn_shared.hip, topn_deep.hip, topn_quota.hip, topn_weighted.hip) ----
// the three parts every scratch layout of theirs has: the chunk's rows of A and its exclusion lists
struct TbChunkDev { unsigned *users, *ex_indptr, *ex_indices; };
template <class Layout> TbChunkDev tb_chunk_dev(unsigned char* base, const Layout& L)
{
    return { (unsigned*)(base + L.users), (unsigned*)(base + L.ex_indptr), (unsigned*)(base + L.ex_indices) };
}

// Cuts the chunk that starts at user u0 -- up to chunk_users users whose exclusion lists fit idx_cap indices together -- and stages it:
// the users' rows of A (users[i], or i itself when compact_A) go to dev.users, their exclusion test to x (tb_stage_excl).  u1: the chunk's
// end, nx: its exclusion indices; hu, hp, hx: staging the caller keeps between chunks.  0, or 1 (a device error; a single row longer
// than idx_cap, which the checks rule out).
inline int tb_stage_chunk(size_t& u1, size_t& nx, TbExcl& x, size_t u0, size_t n_users, size_t chunk_users, size_t idx_cap,
                          const sparse_ix* excl_indptr, const sparse_ix* excl_indices, const sparse_ix* users, bool compact_A,
                          const PmfTopnSeen* seen, const TbChunkDev& dev, std::vector<unsigned>& hu, std::vector<unsigned>& hp,
                          std::vector<unsigned>& hx, hipStream_t stream)
{
    u1 = u0;
    nx = 0;
    while (u1 < n_users && u1 - u0 < chunk_users) {
        const size_t len = excl_indptr ? (size_t)excl_indptr[u1 + 1] - (size_t)excl_indptr[u1] : 0;
        if (u1 > u0 && nx + len > idx_cap) break;
        nx += len;
        u1++;
    }
    if (nx > idx_cap) return 1;
    const size_t nu = u1 - u0;
    hu.resize(nu);
    for (size_t i = 0; i < nu; i++) hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
    TB_TRY(pmf_upload(dev.users, hu.data(), nu * sizeof(unsigned), stream));
    TB_TRY(tb_stage_excl(x, seen, excl_indptr, excl_indices, u0, nu, nx, dev.ex_indptr, dev.ex_indices, hp, hx, stream));
    return 0;
}

// A chunk's results, nu rows of n_top from user u0 on: the items widened to out_ix (an empty entry becomes POISMF_HIP_TOPN_NONE) and,
// when asked for, the scores to out_score.  hix: staging the caller keeps between chunks.  0, or 1 on a device error.
inline int tb_fetch_results(size_t u0, size_t nu, size_t n_top, const unsigned* d_out_ix, const real_t* d_out_score, std::vector<unsigned>& hix,
                            sparse_ix* out_ix, real_t* out_score, hipStream_t stream)
{
    hix.resize(nu * n_top);
    TB_TRY(pmf_download(hix.data(), d_out_ix, nu * n_top * sizeof(unsigned), stream));
    for (size_t i = 0; i < nu * n_top; i++) out_ix[u0 * n_top + i] = hix[i] == TB_NONE ? POISMF_HIP_TOPN_NONE : (sparse_ix)hix[i];
    if (out_score != nullptr) TB_TRY(pmf_download(out_score + u0 * n_top, d_out_score, nu * n_top * sizeof(real_t), stream));
    return 0;
}

// The drop-in entry points: B and either all of A or (when that is less) the batch's rows go to the device of POISMF_HIP_DEVICE,
// run(stream, dA, dB, compact, &d_scratch, &scratch_cap) gives the return code, and everything is freed again.
template <class Run>
int tb_dropin(const real_t* A, const real_t* B, size_t k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users, Run run)
{
    const int device = pmf_env_device();
    if (hipSetDevice(device) != hipSuccess) return 1;
    const hipStream_t st = nullptr;
    const bool compact = n_users < dimA;
    real_t *dA = nullptr, *dB = nullptr;
    void* d_scratch = nullptr;
    size_t scratch_cap = 0;
    int rc = 1;
    do {
        const size_t rowsA = compact ? n_users : dimA;
        if (pmf_alloc(&dA, rowsA * k * sizeof(real_t) + 16, st) != hipSuccess || pmf_alloc(&dB, dimB * k * sizeof(real_t) + 16, st) != hipSuccess) break;
        if (compact) {
            std::vector<real_t> rows;
            try { rows.resize(n_users * k); } catch (const std::bad_alloc&) { break; }
            for (size_t i = 0; i < n_users; i++) memcpy(rows.data() + i * k, A + (size_t)users[i] * k, k * sizeof(real_t));
            if (pmf_upload_big(dA, rows.data(), rowsA * k * sizeof(real_t), device, st) != hipSuccess) break;
        } else if (pmf_upload_big(dA, A, rowsA * k * sizeof(real_t), device, st) != hipSuccess) break;
        if (pmf_upload_big(dB, B, dimB * k * sizeof(real_t), device, st) != hipSuccess) break;
        rc = run(st, dA, dB, compact, &d_scratch, &scratch_cap);
    } while (0);
    pmf_free(dA, st);
    pmf_free(dB, st);
    pmf_free(d_scratch, st);
    return rc;
}

}  // namespace
