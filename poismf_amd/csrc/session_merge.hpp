// session_merge.hpp -- what the two units that change a resident session's matrix share (session_update.hip: X += D, include/poismf_hip.h
// section 2b; session_remove.hip: X -= D, section 2c): the search that places D's cells in the resident rows, the chunking of the pass over
// the resident entries, the scratch of one orientation's pass and the host-side eligibility helpers.  Everything is in an anonymous namespace:
// each unit gets its own instance, and none is visible outside it.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace
