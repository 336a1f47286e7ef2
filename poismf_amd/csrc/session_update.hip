// session_update.hip -- a resident session takes new counts (include/poismf_hip.h section 2b): X += D merged into the resident CSR and CSC
// on the device (locate, scan, scatter, place -- no resident array comes to the host and nothing is sorted again), the download of a half's
// matrix, and a half-sweep over listed rows (a view of the half with a permutation, descriptors and bins of its own: half_sweep.hip runs it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <vector>

#include "session_merge.hpp"

extern "C" {

int poismf_hip_session_add_coo(poismf_hip_session* s, const sparse_ix* row, const sparse_ix* col, const real_t* val, size_t n, size_t* n_new_cells)
{
    if (n_new_cells != nullptr) *n_new_cells = 0;
    if (n == 0) return 0;
    if (s == nullptr || row == nullptr || col == nullptr || val == nullptr || n > 0xffffffffull) return 1;
    for (size_t i = 0; i < n; i++)
        if ((long long)row[i] < 0 || (size_t)row[i] >= s->dimA || (long long)col[i] < 0 || (size_t)col[i] >= s->dimB) return 3;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(val[i]) || !(val[i] > (real_t)0)) return 4;
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (const int e = eligible(s)) return e;
    std::vector<unsigned> rows, cols, h32;
    try { rows = distinct_sorted(row, n, s->dimA); cols = distinct_sorted(col, n, s->dimB); h32.resize(n); } catch (const std::bad_alloc&) { return 1; }
    Scratch sc(s->stream);
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    if (upload_cells(sc, row, col, val, n, h32, &d_row, &d_col, &d_val)) return 1;
    size_t fresh[2] = { 0, 0 };
    const int rc = both_halves(s, [&](int which, Half& h, bool* swapped) {
        const int r = merge_half(s, h, which ? d_row : d_col, which ? d_col : d_row, d_val, n, which ? &rows : &cols, &fresh[which]);
        *swapped = r == 0;   // (a merge that succeeds has swapped)
        return r;
    });
    if (rc == 0 && n_new_cells != nullptr) *n_new_cells = fresh[1];
    return rc;
}

int poismf_hip_session_get_matrix(poismf_hip_session* s, int which, sparse_ix* indptr, sparse_ix* indices, real_t* values)
{
    if (s == nullptr) return 1;
    const Half& h = s->half[which ? 1 : 0];
    if (h.d_indptr == nullptr) return 1;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nloc = h.row_end - h.row_begin;
    try {
        if (indptr != nullptr) {
            std::vector<u64> ip(nloc + 1);
            HIP_TRY(pmf_download(ip.data(), h.d_indptr, sizeof(u64) * (nloc + 1), s->stream));
            for (size_t i = 0; i <= nloc; i++) indptr[i] = (sparse_ix)ip[i];
        }
        if (indices != nullptr && h.nnz > 0) {
            std::vector<unsigned> ix(h.nnz);
            HIP_TRY(pmf_download_big(ix.data(), h.d_indices, sizeof(unsigned) * h.nnz, s->device, s->stream));
            for (size_t i = 0; i < h.nnz; i++) indices[i] = (sparse_ix)ix[i];
        }
    } catch (const std::bad_alloc&) { return 1; }
    if (values != nullptr && h.nnz > 0) HIP_TRY(pmf_download_big(values, h.d_values, sizeof(real_t) * h.nnz, s->device, s->stream));
    return 0;
}

int poismf_hip_half_sweep_rows(poismf_hip_session* s, int which, const sparse_ix* rows, size_t n_rows, const poismf_hip_params* p, real_t step_size,
                               real_t cnst_div, size_t* n_unchanged)
{
    if (n_unchanged != nullptr) *n_unchanged = 0;
    if (n_rows == 0) return 0;
    if (s == nullptr || rows == nullptr || p == nullptr) return 1;
    which = which ? 1 : 0;
    const Half& h = s->half[which];
    if (h.d_indptr == nullptr) return 1;
    const size_t nloc = h.row_end - h.row_begin;
    std::vector<unsigned> local(n_rows), len(n_rows), order(n_rows);
    {
        // distinct and inside the shard: two workgroups updating one row in place would race
        std::vector<bool> taken(nloc, false);
        for (size_t i = 0; i < n_rows; i++) {
            if ((long long)rows[i] < 0 || (size_t)rows[i] < h.row_begin || (size_t)rows[i] >= h.row_end) return 3;
            const size_t l = (size_t)rows[i] - h.row_begin;
            if (taken[l]) return 3;
            taken[l] = true;
            local[i] = (unsigned)l;
        }
    }
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    Half v;   // the view: the half's matrix and counters, a permutation, descriptors and one segment of its own
    v.dimM = h.dimM; v.dimF = h.dimF; v.row_begin = h.row_begin; v.row_end = h.row_end; v.nnz = h.nnz; v.x_positive = h.x_positive;
    v.d_indptr = h.d_indptr; v.d_indices = h.d_indices; v.d_values = h.d_values; v.d_eval_rows = h.d_eval_rows; v.d_dec_rows = h.d_dec_rows;
    Scratch sc(s->stream);   // (owns the view's permutation and descriptors: they go when this call returns)
    unsigned* d_len = nullptr;
    HIP_TRY(sc.get(&v.d_perm, n_rows));
    HIP_TRY(sc.get(&v.d_desc, n_rows));
    HIP_TRY(sc.get(&d_len, n_rows));
    HIP_TRY(pmf_upload(v.d_perm, local.data(), sizeof(unsigned) * n_rows, s->stream));
    hipLaunchKernelGGL(rows_len_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s->stream, h.d_indptr, v.d_perm, n_rows, false, d_len);
    HIP_TRY(pmf_download(len.data(), d_len, sizeof(unsigned) * n_rows, s->stream));
    // longest first, equal lengths by row number: the order finish_half gives a whole half
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return len[a] != len[b] ? len[a] > len[b] : local[a] < local[b]; });
    std::vector<unsigned> perm(n_rows), slen(n_rows);
    for (size_t i = 0; i < n_rows; i++) { perm[i] = local[order[i]]; slen[i] = len[order[i]]; }
    HIP_TRY(pmf_upload(v.d_perm, perm.data(), sizeof(unsigned) * n_rows, s->stream));
    if (row_desc_launch(h.d_indptr, v.d_perm, n_rows, v.d_desc, s->stream)) return 1;
    v.segs.push_back({ 0u, (unsigned)n_rows, bins_of(slen.data(), 0, n_rows) });
    if (half_sweep_impl(s, which, p, step_size, cnst_div, n_unchanged, nullptr, (real_t)0, (real_t)1, -1, &v)) return 1;
    HIP_TRY(hipStreamSynchronize(s->stream));   // (the launches read the view's arrays, which go now)
    return 0;
}

}  // extern "C"
