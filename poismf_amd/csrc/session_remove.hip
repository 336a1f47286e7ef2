// session_remove.hip -- a resident session gives counts back (include/poismf_hip.h section 2c): X -= D on the resident CSR and CSC on the
// device (locate, decide, scan, compact, place -- the inverse of session_update.hip's merge, on the pieces of session_merge.hpp), and the
// removal of whole rows of either half, whose cell list is expanded on the device from the resident rows themselves.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "session_merge.hpp"

namespace {

// ---- the removal from one orientation -------------------------------------------------------------------------------------------------
// After upd_locate_kernel a cell e of D is ABSENT (isnew) or a HIT on entry lb[e] of resident row rowof[e].  A hit is GONE when its entry
// leaves the matrix.  G is the exclusive scan of "gone" over D's cells, so G[dptr[r]] gone cells precede row r: the new row pointers need
// no scan over the rows.

// One lane per cell of D.  A hit takes ONE rounded subtraction nv = x - d and is gone unless nv > 0 (remove_all: gone whatever it holds);
// nv takes d's place in dval for the place kernel.  count[0] += absent cells.
template <class T>
__global__ __launch_bounds__(256) void rem_decide_kernel(const unsigned* rowof, const unsigned* lb, const unsigned* isnew, size_t u, const u64* indptr,
                                                         const T* values, int remove_all, T* dval, unsigned* gone, unsigned* count)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x) {
        if (isnew[e]) { gone[e] = 0u; atomicAdd(count, 1u); continue; }
        const T nv = values[indptr[rowof[e]] + lb[e]] - dval[e];
        dval[e] = nv;
        gone[e] = (remove_all || !(nv > (T)0)) ? 1u : 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) gone[u] = 0u;   // (the scan runs over u + 1 values: G[u] is the number of gone cells)
}

// The gone cells' places in their rows side by side, in D's order (strictly ascending within a row): what the compaction searches.
__global__ __launch_bounds__(256) void rem_gonepos_kernel(const unsigned* lb, const unsigned* gone, const unsigned* G, size_t u, unsigned* gonepos)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x)
        if (gone[e]) gonepos[G[e]] = lb[e];
}

__global__ __launch_bounds__(256) void rem_indptr_kernel(const u64* indptr, const u64* dptr, const unsigned* G, size_t dimM, u64* out)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= dimM; r += (size_t)gridDim.x * blockDim.x) out[r] = indptr[r] - G[dptr[r]];
}

// The bandwidth kernel: every resident entry that stays moves LEFT to its new place.  It mirrors upd_scatter_kernel: the resident arrays are
// walked in chunks of UPD_CHUNK consecutive entries, a workgroup per chunk in a grid-stride loop, so a row of millions of entries is cut
// over many workgroups like any other range.  Per chunk ONE search finds the touched rows [t_lo, t_hi) that overlap it -- none for most
// chunks of a small D: the chunk is then a shift left by one constant.  An entry p outside every touched row moves by the gone cells of the
// touched rows before it; entry j of touched row t moves by Gx[t] + #{gone places of the row < j}, a search in the row's slice of gonepos,
// and is dropped when j is itself a gone place.  Loads of a thread's UPD_PER entries are issued together, lanes on consecutive entries (the
// loads are the aligned side, as in the scatter); nothing waits for another workgroup.  Every store goes to p - shift with shift <= the gone
// cells at or before p, so it stays inside [0, nnz - all gone cells).
template <class T>
__global__ __launch_bounds__(256) void rem_compact_kernel(const unsigned* __restrict__ indices, const T* __restrict__ values, size_t nnz,
                                                          const u64* __restrict__ ta, const u64* __restrict__ tb, const unsigned* __restrict__ Gx,
                                                          size_t nT, const unsigned* __restrict__ gonepos, unsigned* __restrict__ out_indices,
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
        if (t_lo == t_hi || Gx[t_lo] == Gx[t_hi]) {   // no touched row here, or none that loses a cell
            const size_t shift = Gx[t_lo];
#pragma unroll
            for (int q = 0; q < UPD_PER; q++) {
                const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
                if (p < c1) { out_indices[p - shift] = ix[q]; out_values[p - shift] = v[q]; }
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
            if (p >= c1) continue;
            size_t lo = t_lo, hi = t_hi;   // the first touched row of the chunk's that begins behind p
            while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (ta[mid] <= p) lo = mid + 1; else hi = mid; }
            size_t shift = Gx[lo];
            if (lo > t_lo && p < tb[lo - 1]) {   // inside touched row lo - 1: its gone places before this entry count, its own drops it
                const size_t t = lo - 1;
                const unsigned j = (unsigned)(p - ta[t]);
                size_t a = Gx[t];
                const size_t end = Gx[t + 1];
                size_t b = end;
                while (a < b) { const size_t mid = a + (b - a) / 2; if (gonepos[mid] < j) a = mid + 1; else b = mid; }
                if (a < end && gonepos[a] == j) continue;
                shift = a;
            }
            out_indices[p - shift] = ix[q];
            out_values[p - shift] = v[q];
        }
    }
}

// One lane per cell of D.  A hit that stays has lb resident entries before it in its row, of which G[e] - G[dptr[r]] are gone (the gone
// cells before it in D's row are exactly those at smaller places): it writes nv over the entry the compaction has moved there.
template <class T>
__global__ __launch_bounds__(256) void rem_place_kernel(const u64* dptr, const T* dval, size_t u, const unsigned* rowof, const unsigned* lb,
                                                        const unsigned* isnew, const unsigned* gone, const unsigned* G, const u64* new_indptr,
                                                        T* out_values)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x) {
        if (isnew[e] || gone[e]) continue;
        const unsigned r = rowof[e];
        out_values[new_indptr[r] + lb[e] - (G[e] - G[dptr[r]])] = dval[e];
    }
}

// D (n triplets on the device, major / minor as this half sees them; d_val == nullptr: the cells go outright; `touched`: D's distinct major
// indices, ascending, or nullptr: found on the device from D's row pointers) taken out of half h: new arrays are built beside the resident
// ones and take their place only when everything has succeeded.  0, 1, or 6: strict and a cell is absent (nothing written).
int remove_half(poismf_hip_session* s, Half& h, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n,
                const std::vector<unsigned>* touched, int strict, size_t* n_removed, size_t* n_absent)
{
    const hipStream_t st = s->stream;
    const size_t dimM = h.dimM;
    MergeScratch m(st);
    HIP_TRY(pmf_alloc(&m.dptr, sizeof(u64) * (dimM + 1), st));
    HIP_TRY(pmf_alloc(&m.dmin, sizeof(unsigned) * n, st));
    HIP_TRY(pmf_alloc(&m.dval, sizeof(real_t) * n, st));
    real_t* d_fill = nullptr;   // (the conversion sorts values along: cells that go outright carry zeros nobody reads)
    if (d_val == nullptr) {
        HIP_TRY(pmf_alloc(&d_fill, sizeof(real_t) * n, st));
        if (hipMemsetAsync(d_fill, 0, sizeof(real_t) * n, st) != hipSuccess) { pmf_free(d_fill, st); return 1; }
    }
    size_t u = 0;
    const int conv = poismf_hip_device_coo_to_cs(d_major, d_minor, d_val != nullptr ? d_val : d_fill, n, 0, dimM, m.dmin, m.dval, m.dptr, &u, st);
    pmf_free(d_fill, st);
    if (conv) return 1;
    HIP_TRY(pmf_alloc(&m.rowof, sizeof(unsigned) * u, st));
    HIP_TRY(pmf_alloc(&m.lb, sizeof(unsigned) * u, st));
    HIP_TRY(pmf_alloc(&m.isnew, sizeof(unsigned) * (u + 1), st));
    HIP_TRY(pmf_alloc(&m.gone, sizeof(unsigned) * (u + 1), st));
    HIP_TRY(pmf_alloc(&m.G, sizeof(unsigned) * (u + 1), st));
    HIP_TRY(pmf_alloc(&m.count, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(m.count, 0, sizeof(u64), st));
    hipLaunchKernelGGL(upd_locate_kernel, dim3(grid_for(u)), dim3(256), 0, st, m.dptr, m.dmin, u, dimM, h.d_indptr, h.d_indices, m.rowof, m.lb, m.isnew);
    hipLaunchKernelGGL((rem_decide_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, m.rowof, m.lb, m.isnew, u, h.d_indptr, h.d_values,
                       d_val == nullptr ? 1 : 0, m.dval, m.gone, m.count);
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, m.gone, m.G, 0u, u + 1, rocprim::plus<unsigned>(), st));
    HIP_TRY(pmf_alloc(&m.tmp, tmp_bytes ? tmp_bytes : 16, st));
    HIP_TRY(rocprim::exclusive_scan(m.tmp, tmp_bytes, m.gone, m.G, 0u, u + 1, rocprim::plus<unsigned>(), st));
    unsigned ngone = 0, absent = 0;
    HIP_TRY(pmf_download(&ngone, m.G + u, sizeof(unsigned), st));
    HIP_TRY(pmf_download(&absent, m.count, sizeof(unsigned), st));
    *n_removed = ngone;
    *n_absent = absent;
    if (strict && absent > 0) return 6;
    if (absent == u) return 0;   // no listed cell is stored: the half stays as it is
    // the touched rows: the caller's list, or the rows of D that hold a cell
    size_t nT = 0;
    if (touched != nullptr) {
        nT = touched->size();
        HIP_TRY(pmf_alloc(&m.T, sizeof(unsigned) * nT, st));
        HIP_TRY(pmf_upload(m.T, touched->data(), sizeof(unsigned) * nT, st));
    } else {
        const rocprim::counting_iterator<unsigned> rows(0u);
        size_t* d_nT = reinterpret_cast<size_t*>(m.count);
        HIP_TRY(pmf_alloc(&m.T, sizeof(unsigned) * std::min(dimM, u), st));
        pmf_free(m.tmp, st); m.tmp = nullptr;
        HIP_TRY(rocprim::select(nullptr, tmp_bytes, rows, m.T, d_nT, dimM, RowTouched{ m.dptr }, st));
        HIP_TRY(pmf_alloc(&m.tmp, tmp_bytes ? tmp_bytes : 16, st));
        HIP_TRY(rocprim::select(m.tmp, tmp_bytes, rows, m.T, d_nT, dimM, RowTouched{ m.dptr }, st));
        HIP_TRY(pmf_download(&nT, d_nT, sizeof(size_t), st));
    }
    const size_t nnz_new = h.nnz - ngone;
    HIP_TRY(pmf_alloc(&m.ta, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.tb, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.Sx, sizeof(unsigned) * (nT + 1), st));
    HIP_TRY(pmf_alloc(&m.new_indptr, sizeof(u64) * (dimM + 1), st));
    HIP_TRY(pmf_alloc(&m.newlb, sizeof(unsigned) * (ngone ? ngone : 1), st));   // (gonepos)
    HIP_TRY(pmf_alloc(&m.new_indices, sizeof(unsigned) * (nnz_new ? nnz_new : 1), st));
    HIP_TRY(pmf_alloc(&m.new_values, sizeof(real_t) * (nnz_new ? nnz_new : 1), st));
    hipLaunchKernelGGL(rem_gonepos_kernel, dim3(grid_for(u)), dim3(256), 0, st, m.lb, m.gone, m.G, u, m.newlb);
    hipLaunchKernelGGL(upd_touched_kernel, dim3(grid_for(nT + 1)), dim3(256), 0, st, m.T, nT, m.dptr, m.G, u, h.d_indptr, m.ta, m.tb, m.Sx);
    hipLaunchKernelGGL(rem_indptr_kernel, dim3(grid_for(dimM + 1)), dim3(256), 0, st, h.d_indptr, m.dptr, m.G, dimM, m.new_indptr);
    if (h.nnz > 0) {
        const size_t nchunks = (h.nnz + UPD_CHUNK - 1) / UPD_CHUNK;
        const unsigned grid = (unsigned)std::min<size_t>(nchunks, (size_t)s->num_cu * 8);
        hipLaunchKernelGGL((rem_compact_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indices, h.d_values, h.nnz, m.ta, m.tb, m.Sx, nT, m.newlb,
                           m.new_indices, m.new_values);
    }
    hipLaunchKernelGGL((rem_place_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, m.dptr, m.dval, u, m.rowof, m.lb, m.isnew, m.gone, m.G,
                       m.new_indptr, m.new_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    // the swap: from here on the half is the smaller one
    pmf_free(h.d_indptr, st); pmf_free(h.d_indices, st); pmf_free(h.d_values, st);
    h.d_indptr = m.new_indptr; h.d_indices = m.new_indices; h.d_values = m.new_values;
    m.new_indptr = nullptr; m.new_indices = nullptr; m.new_values = nullptr;
    h.nnz = nnz_new;
    return 0;
}

// Both orientations, the CSR first: d_row / d_col / d_val are n triplets on the device; rows / cols as remove_half's `touched`.
int remove_both(poismf_hip_session* s, const unsigned* d_row, const unsigned* d_col, const real_t* d_val, size_t n, const std::vector<unsigned>* rows,
                const std::vector<unsigned>* cols, int strict, size_t* n_removed, size_t* n_absent)
{
    int rc = 0;
    bool written = false;
    for (int which = 1; which >= 0 && rc == 0; which--) {
        Half& h = s->half[which];
        const int nseg = (int)std::max<size_t>(h.segs.size(), 1);
        const unsigned long long* before = h.d_indptr;
        size_t removed = 0, absent = 0;
        rc = remove_half(s, h, which ? d_row : d_col, which ? d_col : d_row, d_val, n, which ? rows : cols, strict, &removed, &absent);
        if (which) { *n_removed = removed; *n_absent = absent; }
        if (rc == 0 && h.d_indptr != before) { written = true; rc = finish_half(h, s->stream, nseg); }   // (swapped: sorted and binned again)
    }
    if (written) s->topn_indptr.clear();   // exclude_seen reads the shortened rows' pointers
    return rc;
}

// 2b's eligibility rule, in full: 0, 5 or 1 (device error)
int eligible(poismf_hip_session* s)
{
    if (!whole_matrix_halves(s)) return 5;
    for (int which = 0; which < 2; which++) {
        const int asc = rows_ascending(s, which);
        if (asc < 0) return 1;
        if (asc == 0) return 5;
    }
    return 0;
}

// ---- whole rows: their cells as triplets -----------------------------------------------------------------------------------------------
// len[i] = stored cells of listed row i (len[n] = 0 for the scan over n + 1 values)
__global__ __launch_bounds__(256) void rem_rows_len_kernel(const u64* indptr, const unsigned* rows, size_t n, unsigned* len)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (size_t)gridDim.x * blockDim.x)
        len[i] = i < n ? (unsigned)(indptr[rows[i] + 1] - indptr[rows[i]]) : 0u;
}

// One lane per cell e of the listed rows (off: the exclusive scan of their lengths, off[n] = total): its row is the last i with off[i] <= e.
__global__ __launch_bounds__(256) void rem_expand_kernel(const u64* indptr, const unsigned* indices, const unsigned* rows, const unsigned* off, size_t n,
                                                         size_t total, unsigned* major, unsigned* minor)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        size_t lo = 0, hi = n - 1;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (off[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const unsigned r = rows[lo];
        major[e] = r;
        minor[e] = indices[indptr[r] + (e - off[lo])];
    }
}

}  // namespace

extern "C" {

int poismf_hip_session_sub_coo(poismf_hip_session* s, const sparse_ix* row, const sparse_ix* col, const real_t* val, size_t n, int strict,
                               size_t* n_removed, size_t* n_absent)
{
    if (n_removed != nullptr) *n_removed = 0;
    if (n_absent != nullptr) *n_absent = 0;
    if (n == 0) return 0;
    if (s == nullptr || row == nullptr || col == nullptr || n > 0xffffffffull) return 1;
    for (size_t i = 0; i < n; i++)
        if ((long long)row[i] < 0 || (size_t)row[i] >= s->dimA || (long long)col[i] < 0 || (size_t)col[i] >= s->dimB) return 3;
    if (val != nullptr)
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(val[i]) || !(val[i] > (real_t)0)) return 4;
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (const int e = eligible(s)) return e;
    std::vector<unsigned> rows, cols, h32;
    try { rows = distinct_sorted(row, n, s->dimA); cols = distinct_sorted(col, n, s->dimB); h32.resize(n); } catch (const std::bad_alloc&) { return 1; }
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    int rc = 1;
    size_t removed = 0, absent = 0;
    do {
        if (pmf_alloc(&d_row, sizeof(unsigned) * n, s->stream) != hipSuccess || pmf_alloc(&d_col, sizeof(unsigned) * n, s->stream) != hipSuccess) break;
        for (size_t i = 0; i < n; i++) h32[i] = (unsigned)row[i];
        if (pmf_upload(d_row, h32.data(), sizeof(unsigned) * n, s->stream) != hipSuccess) break;
        for (size_t i = 0; i < n; i++) h32[i] = (unsigned)col[i];
        if (pmf_upload(d_col, h32.data(), sizeof(unsigned) * n, s->stream) != hipSuccess) break;
        if (val != nullptr) {
            if (pmf_alloc(&d_val, sizeof(real_t) * n, s->stream) != hipSuccess) break;
            if (pmf_upload(d_val, val, sizeof(real_t) * n, s->stream) != hipSuccess) break;
        }
        rc = remove_both(s, d_row, d_col, d_val, n, &rows, &cols, strict, &removed, &absent);
    } while (0);
    pmf_free(d_row, s->stream);
    pmf_free(d_col, s->stream);
    pmf_free(d_val, s->stream);
    if (rc == 0 && n_removed != nullptr) *n_removed = removed;
    if ((rc == 0 || rc == 6) && n_absent != nullptr) *n_absent = absent;
    return rc;
}

int poismf_hip_session_remove_rows(poismf_hip_session* s, int which, const sparse_ix* rows, size_t n_rows, size_t* n_removed)
{
    if (n_removed != nullptr) *n_removed = 0;
    if (n_rows == 0) return 0;
    if (s == nullptr || rows == nullptr) return 1;
    which = which ? 1 : 0;
    const size_t dim = which ? s->dimA : s->dimB;
    std::vector<unsigned> listed;
    try {
        for (size_t i = 0; i < n_rows; i++)
            if ((long long)rows[i] < 0 || (size_t)rows[i] >= dim) return 3;
        listed = distinct_sorted(rows, n_rows, dim);
    } catch (const std::bad_alloc&) { return 1; }
    if (listed.size() != n_rows) return 3;   // a row is listed twice
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (const int e = eligible(s)) return e;
    const Half& h = s->half[which];
    if (h.nnz > 0xffffffffull) return 1;   // (the cell list of a call holds fewer than 2^32 triplets, as sub_coo's)
    const hipStream_t st = s->stream;
    unsigned *d_rows = nullptr, *d_len = nullptr, *d_off = nullptr, *d_major = nullptr, *d_minor = nullptr;
    void* tmp = nullptr;
    int rc = 1;
    size_t removed = 0, absent = 0;
    do {
        if (pmf_alloc(&d_rows, sizeof(unsigned) * n_rows, st) != hipSuccess || pmf_alloc(&d_len, sizeof(unsigned) * (n_rows + 1), st) != hipSuccess ||
            pmf_alloc(&d_off, sizeof(unsigned) * (n_rows + 1), st) != hipSuccess)
            break;
        if (pmf_upload(d_rows, listed.data(), sizeof(unsigned) * n_rows, st) != hipSuccess) break;
        hipLaunchKernelGGL(rem_rows_len_kernel, dim3(grid_for(n_rows + 1)), dim3(256), 0, st, h.d_indptr, d_rows, n_rows, d_len);
        size_t tmp_bytes = 0;
        if (rocprim::exclusive_scan(nullptr, tmp_bytes, d_len, d_off, 0u, n_rows + 1, rocprim::plus<unsigned>(), st) != hipSuccess) break;
        if (pmf_alloc(&tmp, tmp_bytes ? tmp_bytes : 16, st) != hipSuccess) break;
        if (rocprim::exclusive_scan(tmp, tmp_bytes, d_len, d_off, 0u, n_rows + 1, rocprim::plus<unsigned>(), st) != hipSuccess) break;
        unsigned total = 0;
        if (pmf_download(&total, d_off + n_rows, sizeof(unsigned), st) != hipSuccess) break;
        if (total == 0) { rc = 0; break; }
        if (pmf_alloc(&d_major, sizeof(unsigned) * total, st) != hipSuccess || pmf_alloc(&d_minor, sizeof(unsigned) * total, st) != hipSuccess) break;
        hipLaunchKernelGGL(rem_expand_kernel, dim3(grid_for(total)), dim3(256), 0, st, h.d_indptr, h.d_indices, d_rows, d_off, n_rows, (size_t)total, d_major,
                           d_minor);
        if (hipGetLastError() != hipSuccess) break;
        // the listed rows are this half's touched rows; the other half's are found on the device
        rc = remove_both(s, which ? d_major : d_minor, which ? d_minor : d_major, nullptr, total, which ? &listed : nullptr, which ? nullptr : &listed, 0,
                         &removed, &absent);
    } while (0);
    for (void* p : { (void*)d_rows, (void*)d_len, (void*)d_off, (void*)d_major, (void*)d_minor, tmp }) pmf_free(p, st);
    if (rc == 0 && n_removed != nullptr) *n_removed = removed;
    return rc;
}

}  // extern "C"
