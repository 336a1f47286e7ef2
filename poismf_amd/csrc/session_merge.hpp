// session_merge.hpp -- what the three units that change a resident session's matrix share (session_update.hip: X += D, include/poismf_hip.h
// section 2b; session_remove.hip: X -= D, section 2c; session_grow.hip: new rows, section 2d): the search that places D's cells in the
// resident rows, the chunking of the pass over the resident entries, the scratch of one orientation's pass, the host-side eligibility
// helpers and the merge of one orientation (2b's, which 2d runs for the new rows' cells).  Everything is in an anonymous namespace: each
// unit gets its own instance, and none is visible outside it.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <vector>

#include "session.hpp"
#include "cores.hpp"
#include "tb_batch.hpp"

namespace {

typedef unsigned long long u64;

// D arrives as a CS matrix of the half's shape (dptr [dimM + 1], dmin / dval [u], duplicates summed, rows ascending).  A cell e of D in row
// r has lb[e], its lower bound among the resident row's indices, and is NEW (2b) / ABSENT (2c) unless the entry there is its own.
// One lane per cell of D: its row (D's row pointers searched), the lower bound in the resident row, new or not.
__global__ __launch_bounds__(256) void upd_locate_kernel(const u64* dptr, const unsigned* dmin, size_t u, size_t dimM, const u64* indptr,
                                                         const unsigned* indices, unsigned* rowof, unsigned* lb, unsigned* isnew)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x) {
        size_t lo = 0, hi = dimM;   // the last r with dptr[r] <= e (dptr[r + 1] > e: the row is not empty)
        while (lo < hi) {
            const size_t mid = lo + (hi - lo + 1) / 2;
            if (dptr[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const u64 p0 = indptr[lo], p1 = indptr[lo + 1];
        const unsigned c = dmin[e];
        u64 a = p0, b = p1;
        while (a < b) {
            const u64 mid = a + (b - a) / 2;
            if (indices[mid] < c) a = mid + 1; else b = mid;
        }
        rowof[e] = (unsigned)lo;
        lb[e] = (unsigned)(a - p0);
        isnew[e] = (a < p1 && indices[a] == c) ? 0u : 1u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) isnew[u] = 0u;   // (the scan runs over u + 1 values: S[u] is the number of new cells)
}

// Per touched row t (ascending): where its resident entries begin and end, and the new (2b) / gone (2c) cells before it, from
// their exclusive scan S over D's cells; Sx[nT] = all of them.
__global__ __launch_bounds__(256) void upd_touched_kernel(const unsigned* T, size_t nT, const u64* dptr, const unsigned* S, size_t u, const u64* indptr,
                                                          u64* ta, u64* tb, unsigned* Sx)
{
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t <= nT; t += (size_t)gridDim.x * blockDim.x) {
        if (t == nT) { Sx[t] = S[u]; continue; }
        const unsigned r = T[t];
        ta[t] = indptr[r]; tb[t] = indptr[r + 1]; Sx[t] = S[dptr[r]];
    }
}

// The pass over the resident entries walks them in chunks of UPD_CHUNK consecutive entries, a workgroup of 256 per chunk, UPD_PER per thread.
constexpr int UPD_PER = 16;
constexpr int UPD_CHUNK = 256 * UPD_PER;

unsigned grid_for(size_t n, size_t cap = 4096) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, cap)); }

// Everything one orientation's pass allocates; freed by the destructor whichever way the pass ends.  (gone, G, count: the removal's.)
struct MergeScratch {
    hipStream_t stream;
    u64 *dptr = nullptr, *ta = nullptr, *tb = nullptr, *new_indptr = nullptr;
    unsigned *dmin = nullptr, *rowof = nullptr, *lb = nullptr, *isnew = nullptr, *S = nullptr, *newlb = nullptr, *T = nullptr, *Sx = nullptr;
    unsigned *gone = nullptr, *G = nullptr, *count = nullptr;
    unsigned* new_indices = nullptr;
    real_t *dval = nullptr, *new_values = nullptr;
    void* tmp = nullptr;
    explicit MergeScratch(hipStream_t st) : stream(st) {}
    ~MergeScratch()
    {
        for (void* p : { (void*)dptr, (void*)ta, (void*)tb, (void*)new_indptr, (void*)dmin, (void*)rowof, (void*)lb, (void*)isnew, (void*)S, (void*)newlb,
                         (void*)T, (void*)Sx, (void*)gone, (void*)G, (void*)count, (void*)new_indices, (void*)dval, (void*)new_values, tmp })
            pmf_free(p, stream);
    }
};

// are the rows of half `which` strictly ascending (found out once, kept with the session)?  1 yes, 0 no, -1 device error
int rows_ascending(poismf_hip_session* s, int which)
{
    const Half& h = s->half[which];
    std::vector<u64> unused;
    int* word = which ? &s->csr_rows_sorted : &s->csc_rows_sorted;
    PmfTopnSeen seen = { h.d_indptr, h.d_indices, h.row_begin, h.row_end, &unused, word };
    if (poismf_hip_topn_seen_sorted(seen, s->stream)) return -1;
    return *word;
}

// the distinct values of ix (all below dim), ascending: marks over the dimension, no sort
std::vector<unsigned> distinct_sorted(const sparse_ix* ix, size_t n, size_t dim)
{
    std::vector<unsigned char> mark(dim, 0);
    for (size_t i = 0; i < n; i++) mark[(size_t)ix[i]] = 1;
    std::vector<unsigned> v;
    for (size_t r = 0; r < dim; r++)
        if (mark[r]) v.push_back((unsigned)r);
    return v;
}

// 2b's and 2c's eligibility rule, host part: both shards are the whole matrix and the session has a CSC
bool whole_matrix_halves(const poismf_hip_session* s)
{
    for (int which = 0; which < 2; which++) {
        const Half& h = s->half[which];
        if (h.d_indptr == nullptr || h.row_begin != 0 || h.row_end != h.dimM || h.dimM != (which ? s->dimA : s->dimB)) return false;
    }
    return true;
}

// does row r of D hold a cell?
struct RowTouched {
    const u64* dptr;
    __device__ bool operator()(unsigned r) const { return dptr[r + 1] > dptr[r]; }
};


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

// D (n triplets on the device, major / minor as this half sees them; `touched`: its distinct major indices, ascending, or nullptr: found
// on the device from D's row pointers, as remove_half finds them) merged into half h: new arrays are built beside the resident ones and
// take their place only when everything has succeeded.  0 or 1; *n_new: cells not stored before.
int merge_half(poismf_hip_session* s, Half& h, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n,
               const std::vector<unsigned>* touched, size_t* n_new)
{
    const hipStream_t st = s->stream;
    const size_t dimM = h.dimM;
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
    size_t nT = 0;
    if (touched != nullptr) {
        nT = touched->size();
        HIP_TRY(pmf_alloc(&m.T, sizeof(unsigned) * nT, st));
        HIP_TRY(pmf_upload(m.T, touched->data(), sizeof(unsigned) * nT, st));
    } else {
        const rocprim::counting_iterator<unsigned> rows(0u);
        size_t sel_bytes = 0;
        HIP_TRY(pmf_alloc(&m.T, sizeof(unsigned) * std::min(dimM, u), st));
        HIP_TRY(pmf_alloc(&m.count, sizeof(size_t), st));
        size_t* d_nT = reinterpret_cast<size_t*>(m.count);
        HIP_TRY(rocprim::select(nullptr, sel_bytes, rows, m.T, d_nT, dimM, RowTouched{ m.dptr }, st));
        HIP_TRY(pmf_alloc(&m.tmp, sel_bytes ? sel_bytes : 16, st));
        HIP_TRY(rocprim::select(m.tmp, sel_bytes, rows, m.T, d_nT, dimM, RowTouched{ m.dptr }, st));
        HIP_TRY(pmf_download(&nT, d_nT, sizeof(size_t), st));
        pmf_free(m.tmp, st); m.tmp = nullptr;
    }
    HIP_TRY(pmf_alloc(&m.ta, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.tb, sizeof(u64) * nT, st));
    HIP_TRY(pmf_alloc(&m.Sx, sizeof(unsigned) * (nT + 1), st));
    HIP_TRY(pmf_alloc(&m.new_indptr, sizeof(u64) * (dimM + 1), st));
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

}  // namespace
