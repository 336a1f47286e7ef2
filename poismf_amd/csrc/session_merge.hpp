// session_merge.hpp -- what the four units that change a resident session's matrix share (session_update.hip: X += D, include/poismf_hip.h
// section 2b; session_remove.hip: X -= D, section 2c; session_grow.hip: new rows, section 2d; session_scale.hip: X <- gamma X, section 2e).
// Device side: the row search, the chunking of the pass over the resident entries, the search that places D's cells in the resident rows.
// Host side: the eligibility rule, the owner of a call's device scratch, the two rocPRIM calls (scan, touched rows), the upload of a cell
// list, the front of a cell-driven pass (cells_as_cs, locate_cells, touched_rows), the swap that gives a half its new arrays, the driver over both orientations,
// and the merge of one orientation (2b's, which 2d runs for the new rows' cells).  Everything is in an anonymous namespace: each unit
// gets its own instance, and none is visible outside it.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <new>
#include <vector>

#include "session.hpp"
#include "cores.hpp"
#include "tb_batch.hpp"

namespace {

typedef unsigned long long u64;

// The row of entry e under row pointers ptr: the last r in [lo, hi] with ptr[r] <= e (ptr[r + 1] > e: the row is not empty).  The caller
// knows that ptr[lo] <= e.
template <class P> __device__ __forceinline__ size_t upd_row_of(const P* ptr, size_t lo, size_t hi, u64 e)
{
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (ptr[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// D arrives as a CS matrix of the half's shape (dptr [dimM + 1], dmin / dval [u], duplicates summed, rows ascending).  A cell e of D in row
// r has lb[e], its lower bound among the resident row's indices, and is NEW (2b) / ABSENT (2c) unless the entry there is its own.
// One lane per cell of D: its row (D's row pointers searched), the lower bound in the resident row, new or not.
__global__ __launch_bounds__(256) void upd_locate_kernel(const u64* dptr, const unsigned* dmin, size_t u, size_t dimM, const u64* indptr,
                                                         const unsigned* indices, unsigned* rowof, unsigned* lb, unsigned* isnew)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < u; e += (size_t)gridDim.x * blockDim.x) {
        const size_t lo = upd_row_of(dptr, 0, dimM, e);
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

// (uniform over the workgroup) the touched rows [t_lo, t_hi) that overlap the chunk [c0, c1): t_lo is the first touched row that ends
// behind c0, t_hi the first that begins at or behind c1
__device__ __forceinline__ void upd_chunk_touched(const u64* __restrict__ ta, const u64* __restrict__ tb, size_t nT, size_t c0, size_t c1,
                                                  size_t& t_lo, size_t& t_hi)
{
    size_t lo = 0, hi = nT;
    while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (tb[mid] <= c0) lo = mid + 1; else hi = mid; }
    t_lo = lo;
    hi = nT;
    while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (ta[mid] < c1) lo = mid + 1; else hi = mid; }
    t_hi = lo;
}

// a thread's UPD_PER entries of the chunk [c0, c1): the loads are issued together, lanes on consecutive entries
template <class T>
__device__ __forceinline__ void upd_chunk_load(const unsigned* __restrict__ indices, const T* __restrict__ values, size_t c0, size_t c1,
                                               unsigned (&ix)[UPD_PER], T (&v)[UPD_PER])
{
#pragma unroll
    for (int q = 0; q < UPD_PER; q++) {
        const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
        if (p < c1) { ix[q] = indices[p]; v[q] = values[p]; }
    }
}

unsigned grid_for(size_t n, size_t cap = 4096) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, cap)); }

// len[i] = stored cells of listed row i; zero_behind: len[n] = 0 as well, for a scan over n + 1 values
__global__ __launch_bounds__(256) void rows_len_kernel(const u64* indptr, const unsigned* rows, size_t n, bool zero_behind, unsigned* len)
{
    const size_t end = n + (zero_behind ? 1 : 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += (size_t)gridDim.x * blockDim.x)
        len[i] = i < n ? (unsigned)(indptr[rows[i] + 1] - indptr[rows[i]]) : 0u;
}

// The device scratch of one call or one pass, bound to its stream.  get() allocates through pmf_alloc and remembers the array; the
// destructor frees what is still remembered, whichever way the owner's scope ends; drop() frees one array now; release() hands one over:
// its new owner frees it.  Nothing is pooled or reused.
class Scratch {
    hipStream_t stream_;
    std::vector<void*> owned_;
    bool forget(void* p)
    {
        if (p == nullptr) return false;   // (a null local names no array; a failed get() leaves a null entry that is nobody's)
        const auto it = std::find(owned_.begin(), owned_.end(), p);
        if (it == owned_.end()) return false;
        owned_.erase(it);
        return true;
    }

public:
    explicit Scratch(hipStream_t st) : stream_(st) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch()
    {
        for (void* p : owned_) pmf_free(p, stream_);
    }
    hipStream_t stream() const { return stream_; }
    // *p: n elements of T (pmf_alloc's answer; *p is nullptr when it is not hipSuccess)
    template <class T> hipError_t get(T** p, size_t n)
    {
        *p = nullptr;
        try { owned_.push_back(nullptr); } catch (const std::bad_alloc&) { return hipErrorOutOfMemory; }
        const hipError_t e = pmf_alloc(p, sizeof(T) * n, stream_);
        owned_.back() = *p;
        return e;
    }
    void drop(void* p)
    {
        if (forget(p)) pmf_free(p, stream_);
    }
    template <class T> T* release(T* p)
    {
        forget(p);
        return p;
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

// the eligibility rule, host part: both shards are the whole matrix and the session has a CSC
bool whole_matrix_halves(const poismf_hip_session* s)
{
    for (int which = 0; which < 2; which++) {
        const Half& h = s->half[which];
        if (h.d_indptr == nullptr || h.row_begin != 0 || h.row_end != h.dimM || h.dimM != (which ? s->dimA : s->dimB)) return false;
    }
    return true;
}

// The eligibility rule of sections 2b-2e, in full: 0, 5, or 1 (device error).  The session's device is current.
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

// out = the exclusive scan (sum) of in, n > 0 values on the device; *total = out[n - 1] -- the sum of all when in[n - 1] is the zero the
// callers put there.  The temporary storage lives as long as this call.  0 or 1.
template <class V> int scan_exclusive(Scratch& sc, const V* in, V* out, size_t n, V* total)
{
    const hipStream_t st = sc.stream();
    size_t tmp_bytes = 0;
    char* tmp = nullptr;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, in, out, (V)0, n, rocprim::plus<V>(), st));
    HIP_TRY(sc.get(&tmp, tmp_bytes ? tmp_bytes : 16));
    HIP_TRY(rocprim::exclusive_scan(tmp, tmp_bytes, in, out, (V)0, n, rocprim::plus<V>(), st));
    HIP_TRY(pmf_download(total, out + (n - 1), sizeof(V), st));
    sc.drop(tmp);
    return 0;
}

// does row r of D hold a cell?
struct RowTouched {
    const u64* dptr;
    __device__ bool operator()(unsigned r) const { return dptr[r + 1] > dptr[r]; }
};

// *T (sc's): the rows of D (row pointers dptr [dimM + 1], u cells) that hold a cell, ascending, found on the device; *nT: how many.
// d_nT: 8 bytes on the device for the count, the caller's (the removal has a counter it no longer needs), or nullptr: allocated here.
// 0 or 1.
int touched_rows_on_device(Scratch& sc, const u64* dptr, size_t dimM, size_t u, size_t* d_nT, unsigned** T, size_t* nT)
{
    const hipStream_t st = sc.stream();
    const rocprim::counting_iterator<unsigned> rows(0u);
    size_t tmp_bytes = 0;
    char* tmp = nullptr;
    HIP_TRY(sc.get(T, std::min(dimM, u)));
    if (d_nT == nullptr) HIP_TRY(sc.get(&d_nT, 1));
    HIP_TRY(rocprim::select(nullptr, tmp_bytes, rows, *T, d_nT, dimM, RowTouched{ dptr }, st));
    HIP_TRY(sc.get(&tmp, tmp_bytes ? tmp_bytes : 16));
    HIP_TRY(rocprim::select(tmp, tmp_bytes, rows, *T, d_nT, dimM, RowTouched{ dptr }, st));
    HIP_TRY(pmf_download(nT, d_nT, sizeof(size_t), st));
    sc.drop(tmp);
    return 0;
}

// n cells onto the device, owned by sc: major and minor narrowed to unsigned through h32 (the caller's, [n]: no host allocation here),
// val as it is -- nullptr: *d_val stays nullptr (2c's cells that go outright).  0 or 1.
template <class I>
int upload_cells(Scratch& sc, const I* major, const sparse_ix* minor, const real_t* val, size_t n, std::vector<unsigned>& h32, unsigned** d_major,
                 unsigned** d_minor, real_t** d_val)
{
    const hipStream_t st = sc.stream();
    *d_val = nullptr;
    HIP_TRY(sc.get(d_major, n));
    HIP_TRY(sc.get(d_minor, n));
    if (val != nullptr) HIP_TRY(sc.get(d_val, n));
    for (size_t i = 0; i < n; i++) h32[i] = (unsigned)major[i];
    HIP_TRY(pmf_upload(*d_major, h32.data(), sizeof(unsigned) * n, st));
    for (size_t i = 0; i < n; i++) h32[i] = (unsigned)minor[i];
    HIP_TRY(pmf_upload(*d_minor, h32.data(), sizeof(unsigned) * n, st));
    if (val != nullptr) HIP_TRY(pmf_upload(*d_val, val, sizeof(real_t) * n, st));
    return 0;
}

// The front of a cell-driven pass over a half, what merge_half and remove_half have in common; every array is the scratch owner's.
// Three steps, because the two passes order them differently: the merge puts the touched rows on the device before it launches the
// locate pass (the upload of a list synchronises the stream: it meets an idle one), the removal only behind its decide pass, so that a
// refusal (strict and a cell absent) or a call that finds nothing stored has not paid for them.
struct Located {
    size_t u = 0;                                              // cells_as_cs: D's distinct cells;
    u64* dptr = nullptr;                                       // D as a CS matrix of the half's shape: [dimM + 1],
    unsigned* dmin = nullptr;                                  // [u],
    real_t* dval = nullptr;                                    // [u]
    unsigned *rowof = nullptr, *lb = nullptr, *isnew = nullptr;   // storage for locate_cells' answers: [u], [u], [u + 1]
    unsigned* T = nullptr;                                     // touched_rows: the touched rows, ascending:
    size_t nT = 0;                                             // [nT];
    u64 *ta = nullptr, *tb = nullptr;                          // storage for upd_touched_kernel: [nT], [nT],
    unsigned* Sx = nullptr;                                    // [nT + 1]
};

// D (n triplets on the device, major / minor as a half of dimM rows sees them; d_val == nullptr: the values are zeros nobody reads)
// becomes a CS matrix of the half's shape, with storage for what the locate pass finds.  0 or 1.
int cells_as_cs(Scratch& sc, size_t dimM, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n, Located* L)
{
    const hipStream_t st = sc.stream();
    HIP_TRY(sc.get(&L->dptr, dimM + 1));
    HIP_TRY(sc.get(&L->dmin, n));
    HIP_TRY(sc.get(&L->dval, n));
    real_t* d_fill = nullptr;   // (the conversion sorts values along)
    if (d_val == nullptr) {
        HIP_TRY(sc.get(&d_fill, n));
        HIP_TRY(hipMemsetAsync(d_fill, 0, sizeof(real_t) * n, st));
    }
    if (poismf_hip_device_coo_to_cs(d_major, d_minor, d_val != nullptr ? d_val : d_fill, n, 0, dimM, L->dmin, L->dval, L->dptr, &L->u, st)) return 1;
    sc.drop(d_fill);
    const size_t u = L->u;
    HIP_TRY(sc.get(&L->rowof, u));
    HIP_TRY(sc.get(&L->lb, u));
    HIP_TRY(sc.get(&L->isnew, u + 1));
    return 0;
}

// the locate pass: D's cells are looked up in the resident rows of half h (reads the half, writes nothing of it)
void locate_cells(const Half& h, const Located& L, hipStream_t st)
{
    hipLaunchKernelGGL(upd_locate_kernel, dim3(grid_for(L.u)), dim3(256), 0, st, L.dptr, L.dmin, L.u, h.dimM, h.d_indptr, h.d_indices, L.rowof, L.lb, L.isnew);
}

// D's touched rows on the device -- `touched`: its distinct major indices, ascending, or nullptr: found there from D's row pointers
// (d_nT as touched_rows_on_device's) -- and storage for their bounds.  0 or 1.
int touched_rows(Scratch& sc, size_t dimM, const std::vector<unsigned>* touched, size_t* d_nT, Located* L)
{
    if (touched != nullptr) {
        L->nT = touched->size();
        HIP_TRY(sc.get(&L->T, L->nT));
        HIP_TRY(pmf_upload(L->T, touched->data(), sizeof(unsigned) * L->nT, sc.stream()));
    } else if (touched_rows_on_device(sc, L->dptr, dimM, L->u, d_nT, &L->T, &L->nT)) return 1;
    HIP_TRY(sc.get(&L->ta, L->nT));
    HIP_TRY(sc.get(&L->tb, L->nT));
    HIP_TRY(sc.get(&L->Sx, L->nT + 1));
    return 0;
}

// The one place where a half takes its new arrays: the resident three are freed, the scratch owner hands the new three over.  The new
// arrays are built beside the resident ones; a caller swaps when everything has succeeded, as the last thing before it returns 0.
void swap_in(Half& h, Scratch& sc, u64* indptr, unsigned* indices, real_t* values, size_t nnz_new)
{
    pmf_free(h.d_indptr, sc.stream()); pmf_free(h.d_indices, sc.stream()); pmf_free(h.d_values, sc.stream());
    h.d_indptr = sc.release(indptr); h.d_indices = sc.release(indices); h.d_values = sc.release(values);
    h.nnz = nnz_new;
}

// Both orientations, the CSR first (major = row), then the CSC.  pass(which, h, &swapped) changes one half and answers 0 or its error;
// swapped: the half's arrays are new ones.  A swapped half is sorted and binned again with the segments it had before the change, and
// exclude_seen's copy of the row pointers goes when anything was written.  The first error ends the loop and is the answer.
template <class Pass> int both_halves(poismf_hip_session* s, Pass&& pass)
{
    int rc = 0;
    bool written = false;
    for (int which = 1; which >= 0 && rc == 0; which--) {
        Half& h = s->half[which];
        const int nseg = (int)std::max<size_t>(h.segs.size(), 1);
        bool swapped = false;
        rc = pass(which, h, &swapped);
        if (rc == 0 && swapped) { written = true; rc = finish_half(h, s->stream, nseg); }
    }
    if (written) s->topn_indptr.clear();
    return rc;
}


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
        size_t t_lo, t_hi;
        upd_chunk_touched(ta, tb, nT, c0, c1, t_lo, t_hi);
        unsigned ix[UPD_PER];
        T v[UPD_PER];
        upd_chunk_load(indices, values, c0, c1, ix, v);
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
    Scratch sc(st);
    Located L;
    unsigned *S = nullptr, *newlb = nullptr, *new_indices = nullptr;
    u64* new_indptr = nullptr;
    real_t* new_values = nullptr;
    if (cells_as_cs(sc, dimM, d_major, d_minor, d_val, n, &L)) return 1;
    const size_t u = L.u;
    HIP_TRY(sc.get(&S, u + 1));
    if (touched_rows(sc, dimM, touched, nullptr, &L)) return 1;
    const size_t nT = L.nT;
    HIP_TRY(sc.get(&new_indptr, dimM + 1));
    locate_cells(h, L, st);
    unsigned fresh = 0;
    if (scan_exclusive(sc, L.isnew, S, u + 1, &fresh)) return 1;
    const size_t nnz_new = h.nnz + fresh;
    HIP_TRY(sc.get(&newlb, fresh ? fresh : 1));
    HIP_TRY(sc.get(&new_indices, nnz_new ? nnz_new : 1));
    HIP_TRY(sc.get(&new_values, nnz_new ? nnz_new : 1));
    hipLaunchKernelGGL(upd_newlb_kernel, dim3(grid_for(u)), dim3(256), 0, st, L.lb, L.isnew, S, u, newlb);
    hipLaunchKernelGGL(upd_touched_kernel, dim3(grid_for(nT + 1)), dim3(256), 0, st, L.T, nT, L.dptr, S, u, h.d_indptr, L.ta, L.tb, L.Sx);
    hipLaunchKernelGGL(upd_indptr_kernel, dim3(grid_for(dimM + 1)), dim3(256), 0, st, h.d_indptr, L.dptr, S, dimM, new_indptr);
    if (h.nnz > 0) {
        const size_t nchunks = (h.nnz + UPD_CHUNK - 1) / UPD_CHUNK;
        const unsigned grid = (unsigned)std::min<size_t>(nchunks, (size_t)s->num_cu * 8);
        hipLaunchKernelGGL((upd_scatter_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indices, h.d_values, h.nnz, L.ta, L.tb, L.Sx, nT, newlb,
                           new_indices, new_values);
    }
    hipLaunchKernelGGL((upd_place_kernel<real_t>), dim3(grid_for(u)), dim3(256), 0, st, L.dptr, L.dmin, L.dval, u, L.rowof, L.lb, L.isnew, S, new_indptr,
                       new_indices, new_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    swap_in(h, sc, new_indptr, new_indices, new_values, nnz_new);   // from here on the half is the merged one
    *n_new = fresh;
    return 0;
}

}  // namespace
