// session_update.hip -- a resident session takes new counts (include/poismf_hip.h section 2b): X += D merged into the resident CSR and CSC
// on the device (locate, scan, scatter, place -- no resident array comes to the host and nothing is sorted again), the download of a half's
// matrix, and a half-sweep over listed rows (a view of the half with a permutation, descriptors and bins of its own: half_sweep.hip runs it).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <vector>

#include "session_merge.hpp"

namespace {

// ---- the merge of one orientation -----------------------------------------------------------------------------------------------------
// D arrives as a CS matrix of the half's shape (dptr [dimM + 1], dmin / dval [u], duplicates summed, rows ascending).  A cell e of D in row
// r has lb[e], its lower bound among the resident row's indices, and is NEW unless the entry there is its own.  S is the exclusive scan of
// "new" over D's cells, so S[dptr[r]] new cells precede row r: the new row pointers need no scan over the rows.

// The new cells' lower bounds side by side, in D's order (monotone within a row): what the scatter searches.
__global__ __launch_bounds__(256) void upd_newlb_kernel(const unsigned* lb, const unsigned* isnew, const unsigned* S, size_t u, unsigned* newlb)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x)
        if (isnew[e]) newlb[S[e]] = lb[e];
}

__global__ __launch_bounds__(256) void upd_indptr_kernel(const u64* indptr, const u64* dptr, const unsigned* S, size_t dimM, u64* out)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= dimM; r += (size_t)gridDim.x * blockDim.x) out[r] = indptr[r] + S[dptr[r]];
}

// The bandwidth kernel: every resident entry moves to its new place.  The resident arrays are walked in chunks of UPD_CHUNK consecutive
// entries, a workgroup per chunk in a grid-stride loop, so a row of millions of entries is cut over many workgroups like any other range.
// Per chunk ONE search finds the touched rows [t_lo, t_hi) that overlap it -- none for most chunks of a small D: the chunk is then a shift
// by one constant.  An entry p outside every touched row moves by the new cells of the touched rows before it; entry j of touched row t
// moves by Sx[t] + #{new cells of the row with lb <= j}, a search in the row's slice of newlb.  Loads of a thread's UPD_PER entries are
// issued together, lanes on consecutive entries; nothing waits for another workgroup.
template <class T>
__global__ __launch_bounds__(256) void upd_scatter_kernel(const unsigned* __restrict__ indices, const T* __restrict__ values, size_t nnz,
                                                          const u64* __restrict__ ta, const u64* __restrict__ tb, const unsigned* __restrict__ Sx,
                                                          size_t nT, const unsigned* __restrict__ newlb, unsigned* __restrict__ out_indices,
                                                          T* __restrict__ out_values)
{
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const size_t c0 = ch * (size_t)UPD_CHUNK, c1 = std::min(c0 + (size_t)UPD_CHUNK, nnz);
        // (uniform over the workgroup) t_lo: the first touched row that ends behind c0; t_hi: the first that begins at or behind c1
        size_t t_lo = 0, t_hi = nT;
        {
            size_t lo = 0, hi = nT;
            while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (tb[mid] <= c0) lo = mid + 1; else hi = mid; }
            t_lo = lo;
            hi = nT;
            while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (ta[mid] < c1) lo = mid + 1; else hi = mid; }
            t_hi = lo;
        }
        unsigned ix[UPD_PER];
        T v[UPD_PER];
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
            if (p < c1) { ix[q] = indices[p]; v[q] = values[p]; }
        }
        if (t_lo == t_hi) {
            const size_t shift = Sx[t_lo];
#pragma unroll
            for (int q = 0; q < UPD_PER; q++) {
                const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
                if (p < c1) { out_indices[p + shift] = ix[q]; out_values[p + shift] = v[q]; }
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
            if (p >= c1) continue;
            size_t lo = t_lo, hi = t_hi;   // the first touched row of the chunk's that begins behind p
            while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (ta[mid] <= p) lo = mid + 1; else hi = mid; }
            size_t shift = Sx[lo];
            if (lo > t_lo && p < tb[lo - 1]) {   // inside touched row lo - 1: its new cells at or before this entry come first
                const size_t t = lo - 1;
                const unsigned j = (unsigned)(p - ta[t]);
                size_t a = Sx[t], b = Sx[t + 1];
                while (a < b) { const size_t mid = a + (b - a) / 2; if (newlb[mid] <= j) a = mid + 1; else b = mid; }
                shift = a;
            }
            out_indices[p + shift] = ix[q];
            out_values[p + shift] = v[q];
        }
    }
}

// One lane per cell of D.  Resident entries before it in its row: lb; new cells before it in its row: S[e] - S[dptr[r]] -- and that holds
// for a hit as well (the new cells with lb <= its entry's place are exactly those before it in D's row).  A new cell writes itself there,
// a hit adds its value to the entry the scatter has moved there: one rounded addition, D holds no cell twice.
template <class T>
__global__ __launch_bounds__(256) void upd_place_kernel(const u64* dptr, const unsigned* dmin, const T* dval, size_t u, const unsigned* rowof,
                                                        const unsigned* lb, const unsigned* isnew, const unsigned* S, const u64* new_indptr,
                                                        unsigned* out_indices, T* out_values)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned r = rowof[e];
        const u64 pos = new_indptr[r] + lb[e] + (S[e] - S[dptr[r]]);
        if (isnew[e]) { out_indices[pos] = dmin[e]; out_values[pos] = dval[e]; }
        else out_values[pos] += dval[e];
    }
}

// D (n triplets on the device, major / minor as this half sees them; `touched`: its distinct major indices, ascending) merged into half h:
// new arrays are built beside the resident ones and take their place only when everything has succeeded.  0 or 1; *n_new: cells not stored before.
int merge_half(poismf_hip_session* s, Half& h, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n,
               const std::vector<unsigned>& touched, size_t* n_new)
{
    const hipStream_t st = s->stream;
    const size_t dimM = h.dimM, nT = touched.size();
    MergeScratch m(st);
    HIP_TRY(pmf_alloc(&m.dptr, sizeof(u64) * (dimM + 1), st));
    HIP_TRY(pmf_alloc(&m.dmin, sizeof(unsigned) * n, st));
    HIP_TRY(pmf_alloc(&m.dval, sizeof(real_t) * n, st));
    size_t u = 0;
    if (poismf_hip_device_coo_to_cs(d_major, d_minor, d_val, n, 0, dimM, m.dmin, m.dval, m.dptr, &u, st)) return 1;
    HIP_TRY(pmf_alloc(&m.rowof, sizeof(unsigned) * u, st));
    HIP_TRY(pmf_alloc(&m.lb, sizeof(unsigned) * u, st));
    HIP_TRY(pmf_alloc(&m.isnew, sizeof(unsigned) * (u + 1), st));
    HIP_TRY(pmf_alloc(&m.S, sizeof(unsigned) * (u + 1), st));
    HIP_TRY(pmf_alloc(&m.T, sizeof(unsigned) * nT, st));
    HIP_TRY(pmf_alloc(&m.ta, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.tb, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.Sx, sizeof(unsigned) * (nT + 1), st));
    HIP_TRY(pmf_alloc(&m.new_indptr, sizeof(u64) * (dimM + 1), st));
    HIP_TRY(pmf_upload(m.T, touched.data(), sizeof(unsigned) * nT, st));
    hipLaunchKernelGGL(upd_locate_kernel, dim3(grid_for(u)), dim3(256), 0, st, m.dptr, m.dmin, u, dimM, h.d_indptr, h.d_indices, m.rowof, m.lb, m.isnew);
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, m.isnew, m.S, 0u, u + 1, rocprim::plus<unsigned>(), st));
    HIP_TRY(pmf_alloc(&m.tmp, tmp_bytes ? tmp_bytes : 16, st));
    HIP_TRY(rocprim::exclusive_scan(m.tmp, tmp_bytes, m.isnew, m.S, 0u, u + 1, rocprim::plus<unsigned>(), st));
    unsigned fresh = 0;
    HIP_TRY(pmf_download(&fresh, m.S + u, sizeof(unsigned), st));
    const size_t nnz_new = h.nnz + fresh;
    HIP_TRY(pmf_alloc(&m.newlb, sizeof(unsigned) * (fresh ? fresh : 1), st));
    HIP_TRY(pmf_alloc(&m.new_indices, sizeof(unsigned) * (nnz_new ? nnz_new : 1), st));
    HIP_TRY(pmf_alloc(&m.new_values, sizeof(real_t) * (nnz_new ? nnz_new : 1), st));
    hipLaunchKernelGGL(upd_newlb_kernel, dim3(grid_for(u)), dim3(256), 0, st, m.lb, m.isnew, m.S, u, m.newlb);
    hipLaunchKernelGGL(upd_touched_kernel, dim3(grid_for(nT + 1)), dim3(256), 0, st, m.T, nT, m.dptr, m.S, u, h.d_indptr, m.ta, m.tb, m.Sx);
    hipLaunchKernelGGL(upd_indptr_kernel, dim3(grid_for(dimM + 1)), dim3(256), 0, st, h.d_indptr, m.dptr, m.S, dimM, m.new_indptr);
    if (h.nnz > 0) {
        const size_t nchunks = (h.nnz + UPD_CHUNK - 1) / UPD_CHUNK;
        const unsigned grid = (unsigned)std::min<size_t>(nchunks, (size_t)s->num_cu * 8);
        hipLaunchKernelGGL((upd_scatter_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indices, h.d_values, h.nnz, m.ta, m.tb, m.Sx, nT, m.newlb,
                           m.new_indices, m.new_values);
    }
    hipLaunchKernelGGL((upd_place_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, m.dptr, m.dmin, m.dval, u, m.rowof, m.lb, m.isnew, m.S,
                       m.new_indptr, m.new_indices, m.new_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    // the swap: from here on the half is the merged one
    pmf_free(h.d_indptr, st); pmf_free(h.d_indices, st); pmf_free(h.d_values, st);
    h.d_indptr = m.new_indptr; h.d_indices = m.new_indices; h.d_values = m.new_values;
    m.new_indptr = nullptr; m.new_indices = nullptr; m.new_values = nullptr;
    h.nnz = nnz_new;
    *n_new = fresh;
    return 0;
}

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
            ok = merge_half(s, h, which ? d_row : d_col, which ? d_col : d_row, d_val, n, which ? rows : cols, &fresh[which]) == 0 &&
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
