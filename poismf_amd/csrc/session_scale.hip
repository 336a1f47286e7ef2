// session_scale.hip -- a resident session's counts are scaled and what fades leaves (include/poismf_hip.h section 2e): X <- gamma X with
// per-user and per-item factors on the resident CSR and CSC on the device.  Unlike sections 2b-2d, which are driven by a cell list and
// touch a few rows among many, this touches every entry of both orientations: per orientation one dense pass decides (a keep bit per
// entry, a kept count per chunk), a scan over the chunk counts and one lane per row give the new row pointers, and one pass moves the
// survivors -- or, when no cell leaves, one pass rewrites the values in place and nothing else of the half is touched.  The chunking
// and the host-side eligibility helpers are session_merge.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "session_merge.hpp"

namespace {

// A chunk of UPD_CHUNK consecutive entries overlaps the rows [r_lo, r_lo + nrows): more than UPD_CHUNK of them only across empty rows.
// Up to SCL_STAGE rows have their first entry, relative to the chunk, staged in LDS; beyond that an entry's row is searched in the row
// pointers themselves, between the chunk's first and last row.
constexpr unsigned SCL_STAGE = UPD_CHUNK;
constexpr int SCL_WORDS = UPD_CHUNK / 64;   // keep words of a chunk: word j holds entries [64 j, 64 j + 64) of the chunk, bit = lane

struct ChunkRows {
    size_t r_lo;
    unsigned nrows;
    bool staged;
};

// (uniform over the workgroup) the rows of the entries [c0, c1), c0 < c1 <= nnz: r_lo is the row of entry c0 -- the last r with
// indptr[r] <= c0, which is not empty -- and r_lo + nrows - 1 the row of entry c1 - 1.  Stages s_off[j] = first entry of row r_lo + j
// relative to c0 (0 for the row that began before the chunk) when they fit; the caller puts a barrier behind it.
__device__ __forceinline__ ChunkRows scl_chunk_rows(const u64* __restrict__ indptr, size_t dimM, size_t c0, size_t c1, unsigned* s_off)
{
    const size_t r_lo = upd_row_of(indptr, 0, dimM - 1, c0);
    const size_t r_hi = upd_row_of(indptr, r_lo, dimM - 1, c1 - 1);
    ChunkRows c;
    c.r_lo = r_lo;
    c.nrows = (unsigned)std::min<size_t>(r_hi - r_lo + 1, 0xffffffffu);
    c.staged = r_hi - r_lo + 1 <= SCL_STAGE;
    if (c.staged)
        for (unsigned j = threadIdx.x; j < c.nrows; j += 256) {
            const u64 p = indptr[r_lo + j];
            s_off[j] = p > c0 ? (unsigned)(p - c0) : 0u;
        }
    return c;
}

// the row of entry c0 + e of the chunk: the last row of the chunk's that begins at or before it (rows that begin where the next one
// does are empty and never the last)
__device__ __forceinline__ size_t scl_row_of(const ChunkRows& c, const unsigned* s_off, const u64* __restrict__ indptr, size_t c0, unsigned e)
{
    if (c.staged) {
        unsigned lo = 0, hi = c.nrows - 1;
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo + 1) / 2;
            if (s_off[mid] <= e) lo = mid; else hi = mid - 1;
        }
        return c.r_lo + lo;
    }
    size_t lo = c.r_lo, hi = c.r_lo + c.nrows - 1;   // (upd_row_of's search written out: through the helper scl_inplace_kernel grows)
    const u64 p = c0 + e;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (indptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// nv = ((x * gamma) * user scale) * item scale: three multiplications in this order in BOTH orientations, each rounded once.  The
// major scale is the users' in the CSR (user_major) and the items' in the CSC; an absent vector multiplies by 1, which is exact.
template <class T> __device__ __forceinline__ T scl_value(T x, T gamma, T major, T minor, bool user_major)
{
    T a = x * gamma;
    a = a * (user_major ? major : minor);
    a = a * (user_major ? minor : major);
    return a;
}

// The new value of entry c0 + e of the chunk (value x, index ix): its operands are fetched here -- the major scale through the entry's
// row, the minor one through its index -- for the decide and the in-place pass; the compact pass carries the same three lines itself.
template <class T>
__device__ __forceinline__ T scl_entry(T x, unsigned ix, unsigned e, size_t c0, const ChunkRows& rows, const unsigned* s_off,
                                       const u64* __restrict__ indptr, T gamma, const T* __restrict__ major, const T* __restrict__ minor,
                                       int user_major)
{
    const T M = major != nullptr ? major[scl_row_of(rows, s_off, indptr, c0, e)] : (T)1;
    const T m = minor != nullptr ? minor[ix] : (T)1;
    return scl_value(x, gamma, M, m, user_major != 0);
}

// a thread's UPD_PER entries of the chunk [c0, c1) for the passes that write no index: the values, and the indices only when the
// minor vector is given; 0 behind c1
template <class T>
__device__ __forceinline__ void scl_chunk_load(const unsigned* __restrict__ indices, const T* values, bool with_indices, size_t c0, size_t c1,
                                               unsigned (&ix)[UPD_PER], T (&v)[UPD_PER])
{
#pragma unroll
    for (int q = 0; q < UPD_PER; q++) {
        const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
        ix[q] = 0; v[q] = (T)0;
        if (p < c1) { v[q] = values[p]; if (with_indices) ix[q] = indices[p]; }
    }
}

// The decide pass: reads the values (and the indices when the minor vector is given; looks rows up when the major one is), writes a keep
// bit per entry -- 0 behind nnz in the last chunk's words -- and the kept count of every chunk, and adds the results that are not finite
// to *nonfinite.  kept[nchunks] = 0 for the scan over nchunks + 1 values.
template <class T>
__global__ __launch_bounds__(256) void scl_decide_kernel(const u64* __restrict__ indptr, const unsigned* __restrict__ indices,
                                                         const T* __restrict__ values, size_t nnz, size_t dimM, T gamma,
                                                         const T* __restrict__ major, const T* __restrict__ minor, int user_major, T floor,
                                                         u64* __restrict__ keep, u64* __restrict__ kept, u64* nonfinite)
{
    __shared__ unsigned s_off[SCL_STAGE];
    __shared__ unsigned s_cnt[4];
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned bad = 0;
    for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const size_t c0 = ch * (size_t)UPD_CHUNK, c1 = std::min(c0 + (size_t)UPD_CHUNK, nnz);
        ChunkRows rows = { 0, 1, true };
        if (major != nullptr) {
            rows = scl_chunk_rows(indptr, dimM, c0, c1, s_off);
            __syncthreads();
        }
        unsigned ix[UPD_PER];
        T v[UPD_PER];
        scl_chunk_load(indices, values, minor != nullptr, c0, c1, ix, v);
        unsigned wcnt = 0;
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const unsigned e = (unsigned)q * 256 + threadIdx.x;
            const bool in = c0 + e < c1;
            bool stays = false;
            if (in) {
                const T nv = scl_entry(v[q], ix[q], e, c0, rows, s_off, indptr, gamma, major, minor, user_major);
                if (!isfinite(nv)) bad++;
                stays = nv > floor;
            }
            const u64 word = __ballot(stays);
            if (lane == 0) keep[ch * SCL_WORDS + (size_t)q * 4 + wave] = word;
            wcnt += (unsigned)__popcll(word);
        }
        if (lane == 0) s_cnt[wave] = wcnt;
        __syncthreads();
        if (threadIdx.x == 0) kept[ch] = (u64)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();   // (s_off and s_cnt are the next chunk's from here on)
    }
    if (bad) atomicAdd(nonfinite, (u64)bad);
    if (blockIdx.x == 0 && threadIdx.x == 0) kept[nchunks] = 0;
}

// One lane per row pointer: the survivors before entry indptr[r] are those of the chunks before its chunk -- base, the exclusive scan of
// the chunk counts -- plus the keep bits of its chunk before it.  base[nchunks] = all survivors.
__global__ __launch_bounds__(256) void scl_indptr_kernel(const u64* __restrict__ indptr, size_t dimM, size_t nnz, const u64* __restrict__ keep,
                                                         const u64* __restrict__ base, u64* __restrict__ out)
{
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= dimM; r += (size_t)gridDim.x * blockDim.x) {
        const u64 p = indptr[r];
        if (p >= nnz) { out[r] = base[nchunks]; continue; }
        const size_t ch = p / UPD_CHUNK;
        const unsigned e = (unsigned)(p % UPD_CHUNK);
        const u64* words = keep + ch * SCL_WORDS;
        u64 n = base[ch];
        for (unsigned j = 0; j < e / 64; j++) n += (u64)__popcll(words[j]);
        if (e % 64) n += (u64)__popcll(words[e / 64] & ((1ull << (e % 64)) - 1));
        out[r] = n;
    }
}

// The compact pass: every survivor computes nv again from the same operands -- the same bits -- and goes with its index to base[chunk] +
// the keep bits before it in the chunk: the chunk's words and the exclusive prefix of their popcounts sit in LDS.  Survivors stay in
// their order.  Every store goes below base[nchunks], the length of the new arrays: the bits behind nnz are 0.
template <class T>
__global__ __launch_bounds__(256) void scl_compact_kernel(const u64* __restrict__ indptr, const unsigned* __restrict__ indices,
                                                          const T* __restrict__ values, size_t nnz, size_t dimM, T gamma,
                                                          const T* __restrict__ major, const T* __restrict__ minor, int user_major,
                                                          const u64* __restrict__ keep, const u64* __restrict__ base,
                                                          unsigned* __restrict__ out_indices, T* __restrict__ out_values)
{
    __shared__ unsigned s_off[SCL_STAGE];
    __shared__ u64 s_word[SCL_WORDS];
    __shared__ unsigned s_pre[SCL_WORDS];
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const size_t c0 = ch * (size_t)UPD_CHUNK, c1 = std::min(c0 + (size_t)UPD_CHUNK, nnz);
        ChunkRows rows = { 0, 1, true };
        if (major != nullptr) rows = scl_chunk_rows(indptr, dimM, c0, c1, s_off);
        if (wave == 0) {   // (SCL_WORDS == 64: one word per lane of the first wave, all of its lanes active)
            const u64 word = keep[ch * SCL_WORDS + lane];
            const unsigned n = (unsigned)__popcll(word);
            unsigned incl = n;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d, 64);
                if ((int)lane >= d) incl += t;
            }
            s_word[lane] = word;
            s_pre[lane] = incl - n;
        }
        __syncthreads();
        unsigned ix[UPD_PER];
        T v[UPD_PER];
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const size_t p = c0 + (size_t)q * 256 + threadIdx.x;
            ix[q] = 0; v[q] = (T)0;
            if (p < c1) { ix[q] = indices[p]; v[q] = values[p]; }
        }
        const u64 cbase = base[ch];
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const unsigned e = (unsigned)q * 256 + threadIdx.x;
            const u64 word = s_word[q * 4 + wave];
            if (c0 + e >= c1 || !((word >> lane) & 1ull)) continue;
            // (scl_entry's text written out: through the helper this kernel's instruction count moves)
            const T M = major != nullptr ? major[scl_row_of(rows, s_off, indptr, c0, e)] : (T)1;
            const T m = minor != nullptr ? minor[ix[q]] : (T)1;
            const u64 pos = cbase + s_pre[q * 4 + wave] + (u64)__popcll(word & ((1ull << lane) - 1));
            out_indices[pos] = ix[q];
            out_values[pos] = scl_value(v[q], gamma, M, m, user_major != 0);
        }
        __syncthreads();   // (the LDS arrays are the next chunk's from here on)
    }
}

// The in-place pass, when no cell leaves: only the values are rewritten, each by its own lane.
template <class T>
__global__ __launch_bounds__(256) void scl_inplace_kernel(const u64* __restrict__ indptr, const unsigned* __restrict__ indices, T* values,
                                                          size_t nnz, size_t dimM, T gamma, const T* __restrict__ major,
                                                          const T* __restrict__ minor, int user_major)
{
    __shared__ unsigned s_off[SCL_STAGE];
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const size_t c0 = ch * (size_t)UPD_CHUNK, c1 = std::min(c0 + (size_t)UPD_CHUNK, nnz);
        ChunkRows rows = { 0, 1, true };
        if (major != nullptr) {
            rows = scl_chunk_rows(indptr, dimM, c0, c1, s_off);
            __syncthreads();
        }
        unsigned ix[UPD_PER];
        T v[UPD_PER];
        scl_chunk_load(indices, values, minor != nullptr, c0, c1, ix, v);
#pragma unroll
        for (int q = 0; q < UPD_PER; q++) {
            const unsigned e = (unsigned)q * 256 + threadIdx.x;
            if (c0 + e >= c1) continue;
            values[c0 + e] = scl_entry(v[q], ix[q], e, c0, rows, s_off, indptr, gamma, major, minor, user_major);
        }
        if (major != nullptr) __syncthreads();   // (s_off is the next chunk's from here on)
    }
}

// Half h (nnz > 0) scaled: d_major / d_minor are the scale vectors of its rows / of its indices on the device (nullptr: ones).
// `expect` (the CSC's pass): the count of leaving cells the CSR found; a different one is an error.  0, 1, or 7: some result is not
// finite (nothing written).  *swapped: new arrays took the resident ones' place (the caller sorts and bins the half again).
int scale_half(poismf_hip_session* s, Half& h, int which, real_t gamma, const real_t* d_major, const real_t* d_minor, real_t floor,
               const size_t* expect, size_t* n_gone, bool* swapped)
{
    const hipStream_t st = s->stream;
    const size_t dimM = h.dimM, nnz = h.nnz;
    const size_t nchunks = (nnz + UPD_CHUNK - 1) / UPD_CHUNK;
    const unsigned grid = (unsigned)std::min<size_t>(nchunks, (size_t)s->num_cu * 8);
    Scratch sc(st);
    u64 *keep = nullptr, *kept = nullptr, *base = nullptr, *nonfinite = nullptr, *new_indptr = nullptr;
    unsigned* new_indices = nullptr;
    real_t* new_values = nullptr;
    *swapped = false;
    HIP_TRY(sc.get(&keep, nchunks * SCL_WORDS));
    HIP_TRY(sc.get(&kept, nchunks + 1));
    HIP_TRY(sc.get(&base, nchunks + 1));
    HIP_TRY(sc.get(&nonfinite, 1));
    HIP_TRY(hipMemsetAsync(nonfinite, 0, sizeof(u64), st));
    hipLaunchKernelGGL((scl_decide_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indptr, h.d_indices, h.d_values, nnz, dimM, gamma, d_major,
                       d_minor, which, floor, keep, kept, nonfinite);
    u64 stay = 0, bad = 0;
    if (scan_exclusive(sc, kept, base, nchunks + 1, &stay)) return 1;
    HIP_TRY(pmf_download(&bad, nonfinite, sizeof(u64), st));
    if (stay > nnz) return 1;
    *n_gone = nnz - (size_t)stay;
    if (expect != nullptr) {
        if (bad != 0 || *n_gone != *expect) return 1;   // (the orientations disagree: a bug, not an input error)
    } else if (bad != 0) return 7;
    if (*n_gone == 0) {
        hipLaunchKernelGGL((scl_inplace_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indptr, h.d_indices, h.d_values, nnz, dimM, gamma, d_major,
                           d_minor, which);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        h.x_positive = true;   // (every value is > floor >= 0 now)
        return 0;
    }
    const size_t nnz_new = (size_t)stay;
    HIP_TRY(sc.get(&new_indptr, dimM + 1));
    HIP_TRY(sc.get(&new_indices, nnz_new ? nnz_new : 1));
    HIP_TRY(sc.get(&new_values, nnz_new ? nnz_new : 1));
    hipLaunchKernelGGL(scl_indptr_kernel, dim3(grid_for(dimM + 1)), dim3(256), 0, st, h.d_indptr, dimM, nnz, keep, base, new_indptr);
    hipLaunchKernelGGL((scl_compact_kernel<real_t>), dim3(grid), dim3(256), 0, st, h.d_indptr, h.d_indices, h.d_values, nnz, dimM, gamma, d_major,
                       d_minor, which, keep, base, new_indices, new_values);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    swap_in(h, sc, new_indptr, new_indices, new_values, nnz_new);   // from here on the half is the scaled one
    *swapped = true;
    return 0;
}

// finite and >= 0
bool scale_ok(real_t v) { return std::isfinite(v) && v >= (real_t)0; }

}  // namespace

extern "C" {

int poismf_hip_session_scale(poismf_hip_session* s, real_t gamma, const real_t* row_scale, const real_t* col_scale, real_t floor, size_t* n_removed)
{
    if (n_removed != nullptr) *n_removed = 0;
    if (s == nullptr) return 1;
    if (!scale_ok(gamma) || !scale_ok(floor)) return 4;
    if (row_scale != nullptr)
        for (size_t i = 0; i < s->dimA; i++)
            if (!scale_ok(row_scale[i])) return 4;
    if (col_scale != nullptr)
        for (size_t i = 0; i < s->dimB; i++)
            if (!scale_ok(col_scale[i])) return 4;
    if (s->half[0].nnz == 0 && s->half[1].nnz == 0) return 0;
    if (gamma == (real_t)1 && row_scale == nullptr && col_scale == nullptr && floor == (real_t)0) return 0;
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (const int e = eligible(s)) return e;
    const hipStream_t st = s->stream;
    Scratch sc(st);
    real_t *d_row = nullptr, *d_col = nullptr;
    if (row_scale != nullptr) {
        HIP_TRY(sc.get(&d_row, s->dimA));
        HIP_TRY(pmf_upload(d_row, row_scale, sizeof(real_t) * s->dimA, st));
    }
    if (col_scale != nullptr) {
        HIP_TRY(sc.get(&d_col, s->dimB));
        HIP_TRY(pmf_upload(d_col, col_scale, sizeof(real_t) * s->dimB, st));
    }
    size_t gone = 0;
    // (the CSR comes first: it decides what leaves and whether every result is finite)
    const int rc = both_halves(s, [&](int which, Half& h, bool* swapped) {
        size_t left = 0;
        const int r = scale_half(s, h, which, gamma, which ? d_row : d_col, which ? d_col : d_row, floor, which ? nullptr : &gone, &left, swapped);
        if (which) gone = left;
        return r;
    });
    if (rc == 0 && n_removed != nullptr) *n_removed = gone;
    return rc;
}

}  // extern "C"
