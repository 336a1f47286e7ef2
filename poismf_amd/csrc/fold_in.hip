// fold_in.hip -- new rows against a resident B (include/poismf_hip.h section 1m): the guest of a session (its own rows, factor and
// bookkeeping; the host session's B, padded copy, streams and events), the start rows broadcast on the device, factors_multiple's solve on
// the guest (drivers.hip: fold_in_solve), and the batched top-N / ranks straight off the guest's factors and CSR.  No solver and no tile of
// its own: the only kernel here fills the start rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "session.hpp"
#include "tb_batch.hpp"

namespace {

// every row of M [n x k] = row [k]
__global__ __launch_bounds__(256) void broadcast_row_kernel(const real_t* row, real_t* M, size_t n, int k)
{
    const size_t total = n * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) M[i] = row[i % (size_t)k];
}

// The new rows as the entry points take them: row pointers from a non-negative start that never decrease, arrays where there are nonzeros,
// item indices below dimB.  *ascending: every row strictly ascending (what exclude_own's binary search needs).  0, or 2.  No device call.
int rows_check(const real_t* Xr, const sparse_ix* indptr, const sparse_ix* indices, size_t n_new, size_t dimB, bool* ascending)
{
    *ascending = true;
    if (indptr == nullptr || (long long)indptr[0] < 0 || n_new > 0x7fffffffull || dimB > 0x7fffffffull) return 2;
    for (size_t i = 0; i < n_new; i++)
        if (indptr[i + 1] < indptr[i]) return 2;
    if (indptr[n_new] > indptr[0] && (Xr == nullptr || indices == nullptr)) return 2;
    for (size_t i = 0; i < n_new; i++) {
        const size_t p0 = (size_t)indptr[i], p1 = (size_t)indptr[i + 1];
        for (size_t p = p0; p < p1; p++) {
            if ((long long)indices[p] < 0 || (size_t)indices[p] >= dimB) return 2;
            if (p > p0 && (size_t)indices[p - 1] >= (size_t)indices[p]) *ascending = false;
        }
    }
    return 0;
}

// exclude_own of the top-N: every row keeps n_top admissible items once its own items and its exclusion row are united.  0, or 2.
int own_rows_leave(const sparse_ix* indptr, const sparse_ix* indices, size_t n_new, size_t dimB, size_t n_top, const sparse_ix* excl_indptr,
                   const sparse_ix* excl_indices)
{
    std::vector<size_t> row;
    for (size_t i = 0; i < n_new; i++) {
        const size_t len_o = (size_t)indptr[i + 1] - (size_t)indptr[i];
        const size_t len_e = excl_indptr ? (size_t)excl_indptr[i + 1] - (size_t)excl_indptr[i] : 0;
        if (len_o + len_e <= dimB - n_top) continue;
        row.clear();
        for (size_t p = 0; p < len_o; p++) row.push_back((size_t)indices[(size_t)indptr[i] + p]);
        for (size_t p = 0; p < len_e; p++) row.push_back((size_t)excl_indices[(size_t)excl_indptr[i] + p]);
        std::sort(row.begin(), row.end());
        if ((size_t)(std::unique(row.begin(), row.end()) - row.begin()) > dimB - n_top) return 2;
    }
    return 0;
}

// The session's guest, made by the first call that needs one: what it borrows, and the small arrays a half-sweep wants of its session.
// nullptr on failure.
poismf_hip_session* guest_of(poismf_hip_session* host)
{
    if (host->guest != nullptr) return host->guest;
    poismf_hip_session* g = new (std::nothrow) poismf_hip_session();
    if (!g) return nullptr;
    g->borrows_B = true;
    g->device = host->device; g->num_cu = host->num_cu; g->gate_budget = host->gate_budget;
    g->stream = host->stream; g->owns_stream = false;   // ordered after whatever the host has issued
    g->aux_stream = host->aux_stream; g->ev_fork = host->ev_fork; g->ev_join = host->ev_join;
    g->dimB = host->dimB; g->k = host->k; g->ld = host->ld;
    g->dB = host->dB; g->dBp = host->dBp;
    const size_t k = g->k, slack = k * sizeof(real_t) + 16;
    // (d_partial: the guest never sums columns -- its Bsum is the caller's; the k values stage Amean for the broadcast)
    if (pmf_alloc(&g->d_bsum, k * sizeof(real_t) + slack, g->stream) != hipSuccess || pmf_alloc(&g->d_partial, k * sizeof(real_t), g->stream) != hipSuccess ||
        pmf_alloc(&g->d_counter, sizeof(unsigned), g->stream) != hipSuccess ||
        pmf_alloc(&g->d_queue, sizeof(unsigned) * (MAX_LAUNCHES + 2 * TEAM_LAUNCH_MAX), g->stream) != hipSuccess ||
        pmf_alloc(&g->d_arrive, sizeof(unsigned), g->stream) != hipSuccess ||
        pmf_alloc(&g->d_team_err, TEAM_ERR_WORDS * sizeof(unsigned), g->stream) != hipSuccess ||
        hipMemsetAsync(g->d_team_err, 0, TEAM_ERR_WORDS * sizeof(unsigned), g->stream) != hipSuccess) {
        poismf_hip_session_destroy(g);
        return nullptr;
    }
    host->guest = g;
    return g;
}

// The guest's rows replaced by the caller's: their CSR as the A half, room for their factors (grown, never shrunk), every row at its start
// -- Amean, broadcast on the device -- and the all-zero row behind them.  0 or 1.
int guest_fill(poismf_hip_session* g, const real_t* Xr, const sparse_ix* indptr, const sparse_ix* indices, size_t n_new, const real_t* Amean,
               bool start_at_mean)
{
    const size_t k = g->k, slack = k * sizeof(real_t) + 16;
    free_half(g->half[1], g->stream);
    g->topn_indptr.clear();
    g->csr_rows_sorted = -1;
    if (n_new > g->guest_rows) {
        pmf_free(g->dA, g->stream); pmf_free(g->dAp, g->stream);
        g->dA = g->dAp = nullptr;
        g->guest_rows = 0;
        HIP_TRY(pmf_alloc(&g->dA, n_new * k * sizeof(real_t) + slack, g->stream));
        if (g->ld != 0) {   // (the row kernels store every updated row to both copies; the pad columns stay zero from here)
            const size_t bytes = n_new * g->ld * sizeof(real_t) + g->ld * sizeof(real_t) + 16;
            HIP_TRY(pmf_alloc(&g->dAp, bytes, g->stream));
            HIP_TRY(hipMemsetAsync(g->dAp, 0, bytes, g->stream));
        }
        g->guest_rows = n_new;
    }
    g->dimA = n_new;
    g->padded_fresh[1] = false;
    HIP_TRY(hipMemsetAsync(g->dA, 0, n_new * k * sizeof(real_t) + slack, g->stream));
    if (indptr[n_new] == indptr[0]) return 0;   // every row is empty: zero factors, no launch (quirk Q7)
    if (build_half(g->half[1], g->stream, Xr, indptr, indices, n_new, g->dimB, 0, n_new, g->device)) return 1;
    if (start_at_mean) {
        HIP_TRY(pmf_upload(g->d_partial, Amean, k * sizeof(real_t), g->stream));
        const unsigned blocks = (unsigned)std::min<size_t>((n_new * k + 255) / 256, (size_t)g->num_cu * 16);
        hipLaunchKernelGGL(broadcast_row_kernel, dim3(blocks), dim3(256), 0, g->stream, g->d_partial, g->dA, n_new, (int)k);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the solver arguments of a call, as factors_multiple takes them
struct FoldArgs {
    const real_t *Xr; const sparse_ix *indptr, *indices; size_t n_new;
    const real_t *Bsum, *Amean;
    real_t l2_reg, w_mult, step_size; size_t niter, maxupd; int method; bool limit_step, reuse_mean;
};
FoldArgs fold_args(const real_t* Xr, const sparse_ix* indptr, const sparse_ix* indices, size_t n_new, const real_t* Bsum, const real_t* Amean,
                   const poismf_hip_params* p, size_t niter)
{
    return { Xr, indptr, indices, n_new, Bsum, Amean, p->l2_reg, p->w_mult, p->step_size, niter, p->maxupd, p->method, p->limit_step != 0,
             p->reuse_prev != 0 };
}

// The one core: the host's guest holds the rows and their solved factors, and the stream has been waited for.  Arguments already checked.
// Of the host only padded_fresh[0] may change: the guest's prologue refreshes the borrowed padded copy of B when it was stale.  0 or 1.
int fold_in(poismf_hip_session* host, const FoldArgs& f, poismf_hip_session** out)
{
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(host->device));
    poismf_hip_session* g = guest_of(host);
    if (g == nullptr) return 1;
    if (guest_fill(g, f.Xr, f.indptr, f.indices, f.n_new, f.Amean, f.reuse_mean || f.method != POISMF_TNCG)) return 1;
    *out = g;
    if (g->half[1].nnz == 0) return 0;
    g->padded_fresh[0] = host->padded_fresh[0];
    const int rc = fold_in_solve(g, f.Bsum, f.l2_reg, f.w_mult, f.step_size, f.niter, f.maxupd, f.method, f.limit_step, f.reuse_mean);
    host->padded_fresh[0] = g->padded_fresh[0];
    if (rc) return 1;
    HIP_TRY(hipStreamSynchronize(g->stream));
    return team_check(g);
}

// exclude_own: the guest's CSR as the exclusion lists of users 0 .. n_new-1.  Its row pointers and whether its rows ascend are known from
// the host arrays: nothing is fetched back.  false when the guest holds no nonzero (nothing to exclude, and no CSR on the device).
bool guest_seen(poismf_hip_session* g, const FoldArgs& f, bool ascending, PmfTopnSeen& seen)
{
    const Half& h = g->half[1];
    if (h.nnz == 0) return false;
    g->topn_indptr.resize(f.n_new + 1);
    for (size_t i = 0; i <= f.n_new; i++) g->topn_indptr[i] = (unsigned long long)((size_t)f.indptr[i] - (size_t)f.indptr[0]);
    g->csr_rows_sorted = ascending ? 1 : 0;
    seen = { h.d_indptr, h.d_indices, 0, f.n_new, &g->topn_indptr, &g->csr_rows_sorted };
    return true;
}

int factors_out(poismf_hip_session* g, size_t n_new, real_t* out_A)
{
    if (out_A == nullptr) return 0;
    HIP_TRY(pmf_download_big(out_A, g->dA, n_new * g->k * sizeof(real_t), g->device, g->stream));
    return 0;
}

std::vector<sparse_ix> first_rows(size_t n)
{
    std::vector<sparse_ix> u(n);
    for (size_t i = 0; i < n; i++) u[i] = (sparse_ix)i;
    return u;
}

// The top-N of new rows in its two steps -- the session entry runs both, the drop-in makes its temporary session between them.
// The checks: 0, 1 (host memory) or 2; no device call.  users: 0 .. n_new-1, which the run takes.
int topn_new_check(const FoldArgs& f, size_t dimB, size_t k, size_t n_top, int exclude_own, const sparse_ix* excl_indptr,
                   const sparse_ix* excl_indices, std::vector<sparse_ix>& users, bool& ascending)
{
    if (const int rc = rows_check(f.Xr, f.indptr, f.indices, f.n_new, dimB, &ascending)) return rc;
    try { users = first_rows(f.n_new); } catch (const std::bad_alloc&) { return 1; }
    if (const int rc = poismf_hip_topn_batch_check(users.data(), f.n_new, n_top, f.n_new, dimB, k, excl_indptr, excl_indices)) return rc;
    if (exclude_own && own_rows_leave(f.indptr, f.indices, f.n_new, dimB, n_top, excl_indptr, excl_indices)) return 2;
    return 0;
}
int topn_new_run(poismf_hip_session* s, const FoldArgs& f, const std::vector<sparse_ix>& users, bool ascending, size_t n_top, int exclude_own,
                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score, real_t* out_A)
{
    poismf_hip_session* g = nullptr;
    if (fold_in(s, f, &g)) return 1;
    PmfTopnSeen seen;
    const bool own = exclude_own && guest_seen(g, f, ascending, seen);
    if (const int rc = poismf_hip_topn_batch_run(s->stream, g->dA, s->dB, s->dimB, s->k, true, users.data(), f.n_new, n_top, own ? &seen : nullptr,
                                                 excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score))
        return rc;
    return factors_out(g, f.n_new, out_A);
}

}  // namespace

extern "C" {

int poismf_hip_session_factors_new(poismf_hip_session* s, const real_t* Xr, const sparse_ix* Xr_indptr, const sparse_ix* Xr_indices, size_t n_new,
                                   const real_t* Bsum, const real_t* Amean, const poismf_hip_params* p, size_t niter, real_t* out_A)
{
    if (n_new == 0) return 0;
    if (s == nullptr || p == nullptr || Bsum == nullptr || Amean == nullptr || out_A == nullptr) return 2;
    bool ascending = true;
    if (const int rc = rows_check(Xr, Xr_indptr, Xr_indices, n_new, s->dimB, &ascending)) return rc;
    const FoldArgs f = fold_args(Xr, Xr_indptr, Xr_indices, n_new, Bsum, Amean, p, niter);
    poismf_hip_session* g = nullptr;
    if (fold_in(s, f, &g)) return 1;
    return factors_out(g, n_new, out_A);
}

int poismf_hip_session_topn_new(poismf_hip_session* s, const real_t* Xr, const sparse_ix* Xr_indptr, const sparse_ix* Xr_indices, size_t n_new,
                                const real_t* Bsum, const real_t* Amean, const poismf_hip_params* p, size_t niter, size_t n_top, int exclude_own,
                                const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score, real_t* out_A)
{
    if (n_new == 0) return 0;
    if (s == nullptr || p == nullptr || Bsum == nullptr || Amean == nullptr || out_ix == nullptr) return 2;
    const FoldArgs f = fold_args(Xr, Xr_indptr, Xr_indices, n_new, Bsum, Amean, p, niter);
    std::vector<sparse_ix> users;
    bool ascending = true;
    if (const int rc = topn_new_check(f, s->dimB, s->k, n_top, exclude_own, excl_indptr, excl_indices, users, ascending)) return rc;
    return topn_new_run(s, f, users, ascending, n_top, exclude_own, excl_indptr, excl_indices, out_ix, out_score, out_A);
}

int poismf_hip_session_rank_new(poismf_hip_session* s, const real_t* Xr, const sparse_ix* Xr_indptr, const sparse_ix* Xr_indices, size_t n_new,
                                const real_t* Bsum, const real_t* Amean, const poismf_hip_params* p, size_t niter, const sparse_ix* test_indptr,
                                const sparse_ix* test_indices, int exclude_own, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                unsigned int* out_rank, unsigned int* out_n_adm, real_t* out_A)
{
    if (n_new == 0) return 0;
    if (s == nullptr || p == nullptr || Bsum == nullptr || Amean == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    bool ascending = true;
    if (const int rc = rows_check(Xr, Xr_indptr, Xr_indices, n_new, s->dimB, &ascending)) return rc;
    std::vector<sparse_ix> users;
    try { users = first_rows(n_new); } catch (const std::bad_alloc&) { return 1; }
    if (const int rc = poismf_hip_rank_batch_check(users.data(), n_new, n_new, s->dimB, s->k, test_indptr, test_indices, excl_indptr, excl_indices))
        return rc;
    const FoldArgs f = fold_args(Xr, Xr_indptr, Xr_indices, n_new, Bsum, Amean, p, niter);
    poismf_hip_session* g = nullptr;
    if (fold_in(s, f, &g)) return 1;
    PmfTopnSeen seen;
    const bool own = exclude_own && guest_seen(g, f, ascending, seen);
    if (const int rc = poismf_hip_rank_batch_run(s->stream, g->dA, s->dB, s->dimB, s->k, true, users.data(), n_new, test_indptr, test_indices,
                                                 own ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_rank, out_n_adm))
        return rc;
    return factors_out(g, n_new, out_A);
}

int poismf_hip_topn_new(const real_t* B, const real_t* Bsum, const real_t* Amean, const real_t* Xr, const sparse_ix* Xr_indptr,
                        const sparse_ix* Xr_indices, int k, size_t dimB, size_t n_new, real_t l2_reg, real_t w_mult, real_t step_size, size_t niter,
                        size_t maxupd, int method, bool limit_step, bool reuse_mean, size_t n_top, int exclude_own, const sparse_ix* excl_indptr,
                        const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score, real_t* out_A)
{
    if (n_new == 0) return 0;
    if (k < 1 || B == nullptr || Bsum == nullptr || Amean == nullptr || out_ix == nullptr) return 2;
    const FoldArgs f = { Xr, Xr_indptr, Xr_indices, n_new, Bsum, Amean, l2_reg, w_mult, step_size, niter, maxupd, method, limit_step, reuse_mean };
    std::vector<sparse_ix> users;
    bool ascending = true;
    if (const int rc = topn_new_check(f, dimB, (size_t)k, n_top, exclude_own, excl_indptr, excl_indices, users, ascending)) return rc;
    const int device = pmf_env_device();
    poismf_hip_session* s = session_alloc(device, nullptr, 0, dimB, (size_t)k);   // (no rows of A of its own: the guest's are the call's)
    if (s == nullptr) return 1;
    int rc = pmf_upload_big(s->dB, B, dimB * (size_t)k * sizeof(real_t), device, s->stream) != hipSuccess;
    if (!rc) rc = topn_new_run(s, f, users, ascending, n_top, exclude_own, excl_indptr, excl_indices, out_ix, out_score, out_A);
    poismf_hip_session_destroy(s);
    return rc;
}

}  // extern "C"
