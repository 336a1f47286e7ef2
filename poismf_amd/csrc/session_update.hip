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

namespace {

__global__ __launch_bounds__(256) void rows_len_kernel(const u64* indptr, const unsigned* rows, size_t n, unsigned* len)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        len[i] = (unsigned)(indptr[rows[i] + 1] - indptr[rows[i]]);
}

}  // namespace

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
    if (!whole_matrix_halves(s)) return 5;
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    for (int which = 0; which < 2; which++) {
        const int asc = rows_ascending(s, which);
        if (asc < 0) return 1;
        if (asc == 0) return 5;
    }
    std::vector<unsigned> rows, cols, h32;
    try { rows = distinct_sorted(row, n, s->dimA); cols = distinct_sorted(col, n, s->dimB); h32.resize(n); } catch (const std::bad_alloc&) { return 1; }
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    int rc = 1;
    size_t fresh[2] = { 0, 0 };
    do {
        if (pmf_alloc(&d_row, sizeof(unsigned) * n, s->stream) != hipSuccess || pmf_alloc(&d_col, sizeof(unsigned) * n, s->stream) != hipSuccess ||
            pmf_alloc(&d_val, sizeof(real_t) * n, s->stream) != hipSuccess)
            break;
        for (size_t i = 0; i < n; i++) h32[i] = (unsigned)row[i];
        if (pmf_upload(d_row, h32.data(), sizeof(unsigned) * n, s->stream) != hipSuccess) break;
        for (size_t i = 0; i < n; i++) h32[i] = (unsigned)col[i];
        if (pmf_upload(d_col, h32.data(), sizeof(unsigned) * n, s->stream) != hipSuccess) break;
        if (pmf_upload(d_val, val, sizeof(real_t) * n, s->stream) != hipSuccess) break;
        // one orientation after the other: the CSR (major = row), then the CSC (major = column); each is finished with the segments it had
        bool ok = true;
        for (int which = 1; which >= 0 && ok; which--) {
            Half& h = s->half[which];
            const int nseg = (int)std::max<size_t>(h.segs.size(), 1);
            ok = merge_half(s, h, which ? d_row : d_col, which ? d_col : d_row, d_val, n, which ? &rows : &cols, &fresh[which]) == 0 &&
                 finish_half(h, s->stream, nseg) == 0;
        }
        if (!ok) break;
        rc = 0;
    } while (0);
    pmf_free(d_row, s->stream);
    pmf_free(d_col, s->stream);
    pmf_free(d_val, s->stream);
    s->topn_indptr.clear();   // exclude_seen reads the merged rows' pointers
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
    unsigned* d_len = nullptr;
    int rc = 1;
    do {
        if (pmf_alloc(&v.d_perm, sizeof(unsigned) * n_rows, s->stream) != hipSuccess || pmf_alloc(&v.d_desc, sizeof(RowDesc) * n_rows, s->stream) != hipSuccess ||
            pmf_alloc(&d_len, sizeof(unsigned) * n_rows, s->stream) != hipSuccess)
            break;
        if (pmf_upload(v.d_perm, local.data(), sizeof(unsigned) * n_rows, s->stream) != hipSuccess) break;
        hipLaunchKernelGGL(rows_len_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s->stream, h.d_indptr, v.d_perm, n_rows, d_len);
        if (pmf_download(len.data(), d_len, sizeof(unsigned) * n_rows, s->stream) != hipSuccess) break;
        // longest first, equal lengths by row number: the order finish_half gives a whole half
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return len[a] != len[b] ? len[a] > len[b] : local[a] < local[b]; });
        std::vector<unsigned> perm(n_rows), slen(n_rows);
        for (size_t i = 0; i < n_rows; i++) { perm[i] = local[order[i]]; slen[i] = len[order[i]]; }
        if (pmf_upload(v.d_perm, perm.data(), sizeof(unsigned) * n_rows, s->stream) != hipSuccess) break;
        if (row_desc_launch(h.d_indptr, v.d_perm, n_rows, v.d_desc, s->stream)) break;
        v.segs.push_back({ 0u, (unsigned)n_rows, bins_of(slen.data(), 0, n_rows) });
        if (half_sweep_impl(s, which, p, step_size, cnst_div, n_unchanged, nullptr, (real_t)0, (real_t)1, -1, &v)) break;
        if (hipStreamSynchronize(s->stream) != hipSuccess) break;   // (the launches read the view's arrays, which go now)
        rc = 0;
    } while (0);
    pmf_free(d_len, s->stream);
    pmf_free(v.d_perm, s->stream);
    pmf_free(v.d_desc, s->stream);
    return rc;
}

}  // extern "C"
