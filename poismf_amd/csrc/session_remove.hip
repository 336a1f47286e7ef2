// session_remove.hip -- a resident session gives counts back (include/poismf_hip.h section 2c): X -= D on the resident CSR and CSC on the
// device (locate, decide, scan, compact, place -- the inverse of session_update.hip's merge, on the pieces of session_merge.hpp), and the
// removal of whole rows of either half, whose cell list is expanded on the device from the resident rows themselves.
#include <hip/hip_runtime.h>

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
        size_t t_lo, t_hi;
        upd_chunk_touched(ta, tb, nT, c0, c1, t_lo, t_hi);
        unsigned ix[UPD_PER];
        T v[UPD_PER];
        upd_chunk_load(indices, values, c0, c1, ix, v);
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
// ones and take their place only when everything has succeeded.  0, 1, or 6: strict and a cell is absent (nothing written).  *swapped:
// new arrays took the resident ones' place -- not when no listed cell is stored.
int remove_half(poismf_hip_session* s, Half& h, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n,
                const std::vector<unsigned>* touched, int strict, size_t* n_removed, size_t* n_absent, bool* swapped)
{
    const hipStream_t st = s->stream;
    const size_t dimM = h.dimM;
    Scratch sc(st);
    Located L;
    if (cells_as_cs(sc, dimM, d_major, d_minor, d_val, n, &L)) return 1;
    const size_t u = L.u;
    unsigned *gone = nullptr, *G = nullptr, *gonepos = nullptr, *new_indices = nullptr;
    size_t* count = nullptr;   // 8 bytes: the absent cells (an unsigned, the decide pass's), later the touched rows' count (the select's)
    u64* new_indptr = nullptr;
    real_t* new_values = nullptr;
    HIP_TRY(sc.get(&gone, u + 1));
    HIP_TRY(sc.get(&G, u + 1));
    HIP_TRY(sc.get(&count, 1));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(size_t), st));
    locate_cells(h, L, st);
    hipLaunchKernelGGL((rem_decide_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, L.rowof, L.lb, L.isnew, u, h.d_indptr, h.d_values,
                       d_val == nullptr ? 1 : 0, L.dval, gone, reinterpret_cast<unsigned*>(count));
    unsigned ngone = 0, absent = 0;
    if (scan_exclusive(sc, gone, G, u + 1, &ngone)) return 1;
    HIP_TRY(pmf_download(&absent, count, sizeof(unsigned), st));
    *n_removed = ngone;
    *n_absent = absent;
    if (strict && absent > 0) return 6;
    if (absent == u) return 0;   // no listed cell is stored: the half stays as it is
    if (touched_rows(sc, dimM, touched, count, &L)) return 1;
    const size_t nT = L.nT, nnz_new = h.nnz - ngone;
    HIP_TRY(sc.get(&new_indptr, dimM + 1));
    HIP_TRY(sc.get(&gonepos, ngone ? ngone : 1));
    HIP_TRY(sc.get(&new_indices, nnz_new ? nnz_new : 1));
    HIP_TRY(sc.get(&new_values, nnz_new ? nnz_new : 1));
    hipLaunchKernelGGL(rem_gonepos_kernel, dim3(grid_for(u)), dim3(256), 0, st, L.lb, gone, G, u, gonepos);
    hipLaunchKernelGGL(upd_touched_kernel, dim3(grid_for(nT + 1)), dim3(256), 0, st, L.T, nT, L.dptr, G, u, h.d_indptr, L.ta, L.tb, L.Sx);
    hipLaunchKernelGGL(rem_indptr_kernel, dim3(grid_for(dimM + 1)), dim3(256), 0, st, h.d_indptr, L.dptr, G, dimM, new_indptr);
    if (h.nnz > 0) {
        const size_t nchunks = (h.nnz + UPD_CHUNK - 1) / UPD_CHUNK;
        const unsigned grid = (unsigned)std::min<size_t>(nchunks, (size_t)s->num_cu * 8);
        hipLaunchKernelGGL((rem_compact_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indices, h.d_values, h.nnz, L.ta, L.tb, L.Sx, nT, gonepos,
                           new_indices, new_values);
    }
    hipLaunchKernelGGL((rem_place_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, L.dptr, L.dval, u, L.rowof, L.lb, L.isnew, gone, G, new_indptr,
                       new_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    swap_in(h, sc, new_indptr, new_indices, new_values, nnz_new);   // from here on the half is the smaller one
    *swapped = true;
    return 0;
}

// Both orientations: d_row / d_col / d_val are n triplets on the device; rows / cols as remove_half's `touched`.  The counts are the CSR's.
int remove_both(poismf_hip_session* s, const unsigned* d_row, const unsigned* d_col, const real_t* d_val, size_t n, const std::vector<unsigned>* rows,
                const std::vector<unsigned>* cols, int strict, size_t* n_removed, size_t* n_absent)
{
    return both_halves(s, [&](int which, Half& h, bool* swapped) {
        size_t removed = 0, absent = 0;
        const int rc = remove_half(s, h, which ? d_row : d_col, which ? d_col : d_row, d_val, n, which ? rows : cols, strict, &removed, &absent, swapped);
        if (which) { *n_removed = removed; *n_absent = absent; }
        return rc;
    });
}

// ---- whole rows: their cells as triplets -----------------------------------------------------------------------------------------------

// One lane per cell e of the listed rows (off: the exclusive scan of their lengths, off[n] = total): its row is the last i with off[i] <= e.
__global__ __launch_bounds__(256) void rem_expand_kernel(const u64* indptr, const unsigned* indices, const unsigned* rows, const unsigned* off, size_t n,
                                                         size_t total, unsigned* major, unsigned* minor)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t lo = upd_row_of(off, 0, n - 1, e);
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
    Scratch sc(s->stream);
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    if (upload_cells(sc, row, col, val, n, h32, &d_row, &d_col, &d_val)) return 1;
    size_t removed = 0, absent = 0;
    const int rc = remove_both(s, d_row, d_col, d_val, n, &rows, &cols, strict, &removed, &absent);
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
    Scratch sc(st);
    unsigned *d_rows = nullptr, *d_len = nullptr, *d_off = nullptr, *d_major = nullptr, *d_minor = nullptr;
    HIP_TRY(sc.get(&d_rows, n_rows));
    HIP_TRY(sc.get(&d_len, n_rows + 1));
    HIP_TRY(sc.get(&d_off, n_rows + 1));
    HIP_TRY(pmf_upload(d_rows, listed.data(), sizeof(unsigned) * n_rows, st));
    hipLaunchKernelGGL(rows_len_kernel, dim3(grid_for(n_rows + 1)), dim3(256), 0, st, h.d_indptr, d_rows, n_rows, true, d_len);
    unsigned total = 0;
    if (scan_exclusive(sc, d_len, d_off, n_rows + 1, &total)) return 1;
    if (total == 0) return 0;
    HIP_TRY(sc.get(&d_major, total));
    HIP_TRY(sc.get(&d_minor, total));
    hipLaunchKernelGGL(rem_expand_kernel, dim3(grid_for(total)), dim3(256), 0, st, h.d_indptr, h.d_indices, d_rows, d_off, n_rows, (size_t)total, d_major,
                       d_minor);
    HIP_TRY(hipGetLastError());
    // the listed rows are this half's touched rows; the other half's are found on the device
    size_t removed = 0, absent = 0;
    const int rc = remove_both(s, which ? d_major : d_minor, which ? d_minor : d_major, nullptr, total, which ? &listed : nullptr,
                               which ? nullptr : &listed, 0, &removed, &absent);
    if (rc == 0 && n_removed != nullptr) *n_removed = removed;
    return rc;
}

}  // extern "C"
