// llk.hip -- Poisson log-likelihood of fitted factors on a set of cells (include/poismf_hip.h, section 1e):
//
//   llk = sum_cells [ x log yhat - lgamma(x + 1) [full_llk] ] - M,   yhat = A[i,:] . B[j,:] in double
//   M   = sum_cells yhat                          (include_missing = 0)
//   M   = sum_c (sum_i A[i,c]) (sum_j B[j,c])      (include_missing = 1: every cell of the matrix, missing = 0)
//
// The reference declares eval_llk (ref: src/poismf.h:258-269) and defines it nowhere.  One kernel over
// a CSR serves both the host drop-in (eval_llk, triplets converted on the device by coo_convert.hip) and the session
// (poismf_hip_session_llk, its resident CSR shard and factors).
//
// Work is cut into fixed RANGES of LLK_RANGE consecutive nonzeros, one workgroup each, whatever the row lengths (power-law
// and giant rows balance by construction).  Inside a range each 16-lane group walks a contiguous chunk of LLK_CHUNK
// nonzeros, 16 at a time: lane t finds the row of nonzero t by binary search in indptr and loads its column and value
// (coalesced); then the group computes the 16 dot products one after the other -- the A row stays in registers while the
// row does not change, the B row is gathered by the 16 lanes side by side -- and lane t keeps the t-th, so that the log
// is taken once per nonzero, not once per lane.  The lgamma(x + 1) terms of full_llk, which the factors do not enter, are
// a separate pass over the values with the same ranges.
//
// Deterministic and independent of the grid: a nonzero's place in the arithmetic depends on its position in the CSR
// alone.  Each range writes one fp64 partial (lane sums in chunk order, the wave's fixed DPP tree, the four waves in
// order), and one for its lgamma terms; one workgroup adds each set of partials in a fixed order.  The column sums for include_missing are fp64 sums over fixed
// blocks of LLK_COL_ROWS rows, then over the blocks in order.
#include <cstring>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "wave_ops.hpp"
#include "cores.hpp"

namespace {

using pmf::WAVE;

constexpr int LLK_WG = 256;                        // threads per workgroup
constexpr int LLK_G = 16;                          // lanes per nonzero
constexpr int LLK_RANGE = 4096;                    // nonzeros per range (= workgroup)
constexpr int LLK_CHUNK = LLK_RANGE / (LLK_WG / LLK_G);   // nonzeros per 16-lane group
constexpr int LLK_COL_ROWS = 1024;                 // rows per block of the include_missing column sums
constexpr int LLK_K_MAX = 32 * LLK_G;              // k <= 512 (what a session supports in fp32; fp64 sessions stop at 256)

// largest r in [lo, hi] with indptr[r] <= n (the row that holds nonzero n, given indptr[lo] <= n < indptr[hi + 1])
__device__ __forceinline__ unsigned row_of(const unsigned long long* indptr, unsigned long long n, unsigned lo, unsigned hi)
{
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo + 1) / 2;
        if (indptr[mid] <= n) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// fixed-order sum over the workgroup: the wave's DPP tree, then the waves in order (thread 0 gets the result)
__device__ __forceinline__ double block_sum(double v, double* lds)
{
    v = pmf::wave_sum(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < LLK_WG / WAVE; w++) s += lds[w];
    return s;
}

// One workgroup per range of LLK_RANGE nonzeros.  A: the rows of the CSR ([nrows x k], local row 0 first), B: [dimB x k].
template <int KPL>
__global__ __launch_bounds__(LLK_WG) void llk_range_kernel(const real_t* __restrict__ A, const real_t* __restrict__ B,
                                                           const unsigned long long* __restrict__ indptr, unsigned nrows,
                                                           const unsigned* __restrict__ col, const real_t* __restrict__ val,
                                                           unsigned long long nnz, int k, int include_missing, double* __restrict__ partial)
{
    __shared__ double lds[LLK_WG / WAVE];
    const int sub = (int)(threadIdx.x & (LLK_G - 1));
    const unsigned long long p0 = (unsigned long long)blockIdx.x * LLK_RANGE + (unsigned long long)(threadIdx.x / LLK_G) * LLK_CHUNK;
    const unsigned long long p1 = p0 + LLK_CHUNK < nnz ? p0 + LLK_CHUNK : nnz;
    double acc = 0.0;
    if (p0 < p1) {
        unsigned lo = row_of(indptr, p0, 0, nrows - 1);
        const unsigned hi = row_of(indptr, p1 - 1, lo, nrows - 1);
        unsigned cur = 0xffffffffu;
        real_t a[KPL];
        for (unsigned long long n0 = p0; n0 < p1; n0 += LLK_G) {
            const unsigned long long n = n0 + (unsigned long long)sub;
            const bool live = n < p1;
            unsigned r = lo, j = 0;
            double x = 0.0;
            if (live) {
                r = row_of(indptr, n, lo, hi);
                j = col[n];
                x = (double)val[n];
            }
            const int cnt = p1 - n0 < (unsigned long long)LLK_G ? (int)(p1 - n0) : LLK_G;
            double mine = 0.0;
            for (int t = 0; t < cnt; t++) {
                const unsigned rt = (unsigned)__shfl((int)r, t, LLK_G);
                const unsigned jt = (unsigned)__shfl((int)j, t, LLK_G);
                if (rt != cur) {   // (uniform over the group) a new row: its A row into registers
                    cur = rt;
                    const real_t* ar = A + (size_t)rt * (size_t)k;
#pragma unroll
                    for (int q = 0; q < KPL; q++) {
                        const int c = sub + q * LLK_G;
                        a[q] = c < k ? ar[c] : (real_t)0;
                    }
                }
                const real_t* br = B + (size_t)jt * (size_t)k;
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < KPL; q++) {
                    const int c = sub + q * LLK_G;
                    if (c < k) s = __builtin_fma((double)a[q], (double)br[c], s);
                }
                // (xor butterfly: partner lanes add the same two operands, so all 16 lanes end with the same bits)
                s += __shfl_xor(s, 8, LLK_G);
                s += __shfl_xor(s, 4, LLK_G);
                s += __shfl_xor(s, 2, LLK_G);
                s += __shfl_xor(s, 1, LLK_G);
                if (sub == t) mine = s;
            }
            lo = (unsigned)__shfl((int)r, cnt - 1, LLK_G);
            if (live) {
                double term = x != 0.0 ? x * pmf::d_log(mine) : 0.0;   // (no log for x = 0: such a cell only costs its yhat)
                if (!include_missing) term -= mine;
                acc += term;
            }
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// full_llk: sum of lgamma(x + 1) over the same ranges, one partial each.  A pass of its own over the values: the device library's
// lgamma would raise the gather kernel from 56 to ~200 VGPRs (2 waves per SIMD instead of 8) for a term the factors do not enter.
__global__ __launch_bounds__(LLK_WG) void llk_lgamma_kernel(const real_t* __restrict__ val, unsigned long long nnz, double* __restrict__ partial)
{
    __shared__ double lds[LLK_WG / WAVE];
    const unsigned long long p0 = (unsigned long long)blockIdx.x * LLK_RANGE;
    const unsigned long long p1 = p0 + LLK_RANGE < nnz ? p0 + LLK_RANGE : nnz;
    double acc = 0.0;
    for (unsigned long long n = p0 + threadIdx.x; n < p1; n += LLK_WG) acc += lgamma((double)val[n] + 1.0);
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// include_missing: fp64 column sums over blocks of LLK_COL_ROWS rows (one workgroup per block), then over the blocks in order
__global__ __launch_bounds__(LLK_WG) void llk_colsum_block_kernel(const real_t* __restrict__ M, size_t nrows, int k, double* __restrict__ part)
{
    const size_t r0 = (size_t)blockIdx.x * LLK_COL_ROWS;
    const size_t r1 = std::min(r0 + LLK_COL_ROWS, nrows);
    for (int c = (int)threadIdx.x; c < k; c += LLK_WG) {
        double s = 0.0;
        for (size_t r = r0; r < r1; r++) s += (double)M[r * (size_t)k + c];
        part[(size_t)blockIdx.x * k + c] = s;
    }
}
__global__ __launch_bounds__(LLK_WG) void llk_colsum_final_kernel(const double* __restrict__ part, size_t nblocks, int k, double* __restrict__ out)
{
    for (int c = (int)threadIdx.x; c < k; c += LLK_WG) {
        double s = 0.0;
        for (size_t b = 0; b < nblocks; b++) s += part[b * (size_t)k + c];
        out[c] = s;
    }
}

// out[0] = (sum of the range partials) - (sum of the lgamma partials) - M, each sum in a fixed order
__global__ __launch_bounds__(LLK_WG) void llk_final_kernel(const double* __restrict__ partial, const double* __restrict__ lg_partial, size_t nranges,
                                                           const double* __restrict__ sA, const double* __restrict__ sB, int k, int full_llk,
                                                           int include_missing, double* __restrict__ out)
{
    __shared__ double lds[LLK_WG / WAVE];
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < nranges; i += LLK_WG) acc += partial[i];
    double s = block_sum(acc, lds);
    if (full_llk) {
        __syncthreads();
        acc = 0.0;
        for (size_t i = threadIdx.x; i < nranges; i += LLK_WG) acc += lg_partial[i];
        const double lg = block_sum(acc, lds);
        s -= lg;
    }
    if (threadIdx.x == 0) {
        if (include_missing) {
            double m = 0.0;
            for (int c = 0; c < k; c++) m += sA[c] * sB[c];
            s -= m;
        }
        out[0] = s;
    }
}

struct Layout {   // the scratch array of poismf_hip_llk_enqueue, in doubles
    size_t nranges, nbA, nbB, part, lg, colA, colB, sA, sB, total;
    Layout(size_t nrows, size_t dimB, size_t k, size_t nnz)
    {
        nranges = pmf_ceil_div(nnz, LLK_RANGE);
        nbA = pmf_ceil_div(nrows, LLK_COL_ROWS);
        nbB = pmf_ceil_div(dimB, LLK_COL_ROWS);
        part = 1;                       // [0]: the result
        lg = part + nranges;
        colA = lg + nranges;
        colB = colA + nbA * k;
        sA = colB + nbB * k;
        sB = sA + k;
        total = sB + k;
    }
};

template <int KPL>
void launch_ranges(size_t nranges, hipStream_t stream, const real_t* A, const real_t* B, const unsigned long long* indptr, size_t nrows,
                   const unsigned* col, const real_t* val, size_t nnz, int k, int include_missing, double* partial)
{
    hipLaunchKernelGGL(llk_range_kernel<KPL>, dim3((unsigned)nranges), dim3(LLK_WG), 0, stream, A, B, indptr, (unsigned)nrows, col, val,
                       (unsigned long long)nnz, k, include_missing, partial);
}

}  // namespace

// ---- core on device-resident data (the session and the drop-in below) ----
// Doubles of scratch poismf_hip_llk_enqueue needs.
size_t poismf_hip_llk_scratch(size_t nrows, size_t dimB, size_t k, size_t nnz) { return Layout(nrows, dimB, k, nnz).total; }

// Enqueues the evaluation on `stream`; the result lands in scratch[0].  A: the CSR's rows ([nrows x k], compact), B: [dimB x k];
// indptr: nrows + 1 entries from 0, col < dimB.  Returns 0, or 1 when k is out of range or a launch fails.
int poismf_hip_llk_enqueue(const real_t* A, const real_t* B, size_t nrows, size_t dimB, size_t k, const unsigned long long* indptr,
                           const unsigned* col, const real_t* val, size_t nnz, int full_llk, int include_missing, double* scratch,
                           hipStream_t stream)
{
    if (k < 1 || k > (size_t)LLK_K_MAX || nrows > 0x7fffffffull || nnz > 0xffffffffull) return 1;
    const Layout L(nrows, dimB, k, nnz);
    const int ki = (int)k;
    if (L.nranges > 0) {
        const size_t kpl = pmf_ceil_div(k, LLK_G);
        double* part = scratch + L.part;
        if (kpl <= 1) launch_ranges<1>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
        else if (kpl <= 2) launch_ranges<2>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
        else if (kpl <= 4) launch_ranges<4>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
        else if (kpl <= 8) launch_ranges<8>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
        else if (kpl <= 16) launch_ranges<16>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
        else launch_ranges<32>(L.nranges, stream, A, B, indptr, nrows, col, val, nnz, ki, include_missing, part);
    }
    if (full_llk && L.nranges > 0)
        hipLaunchKernelGGL(llk_lgamma_kernel, dim3((unsigned)L.nranges), dim3(LLK_WG), 0, stream, val, (unsigned long long)nnz, scratch + L.lg);
    if (include_missing) {
        if (L.nbA > 0)
            hipLaunchKernelGGL(llk_colsum_block_kernel, dim3((unsigned)L.nbA), dim3(LLK_WG), 0, stream, A, nrows, ki, scratch + L.colA);
        if (L.nbB > 0)
            hipLaunchKernelGGL(llk_colsum_block_kernel, dim3((unsigned)L.nbB), dim3(LLK_WG), 0, stream, B, dimB, ki, scratch + L.colB);
        hipLaunchKernelGGL(llk_colsum_final_kernel, dim3(1), dim3(LLK_WG), 0, stream, scratch + L.colA, L.nbA, ki, scratch + L.sA);
        hipLaunchKernelGGL(llk_colsum_final_kernel, dim3(1), dim3(LLK_WG), 0, stream, scratch + L.colB, L.nbB, ki, scratch + L.sB);
    }
    hipLaunchKernelGGL(llk_final_kernel, dim3(1), dim3(LLK_WG), 0, stream, scratch + L.part, scratch + L.lg, L.nranges, scratch + L.sA,
                       scratch + L.sB, ki, full_llk, include_missing, scratch);
    return hipGetLastError() != hipSuccess;
}

extern "C" {

long double eval_llk(real_t* A, real_t* B, sparse_ix ixA[], sparse_ix ixB[], real_t* X, size_t nnz, int k, bool full_llk,
                     bool include_missing, size_t dimA, size_t dimB, int nthreads)
{
    (void)nthreads;
    const long double nan = std::numeric_limits<long double>::quiet_NaN();
    if (k < 1 || k > LLK_K_MAX) {
        fprintf(stderr, "eval_llk: k = %d is outside the supported range (1..%d)\n", k, LLK_K_MAX);
        return nan;
    }
    if (dimA > 0x7fffffffull || dimB > 0x7fffffffull || nnz > 0xffffffffull) {
        fprintf(stderr, "eval_llk: dimensions must be below 2^31 and nnz below 2^32\n");
        return nan;
    }
    std::vector<unsigned> hr, hc;
    try { hr.resize(nnz); hc.resize(nnz); } catch (const std::bad_alloc&) { fprintf(stderr, "Error: out of memory.\n"); return nan; }
    for (size_t i = 0; i < nnz; i++) {
        // (an index outside the matrix would become a gather offset into the factors; a negative R index wraps to a huge one)
        if ((size_t)ixA[i] >= dimA || (size_t)ixB[i] >= dimB) {
            fprintf(stderr, "eval_llk: triplet %zu: index (%zu, %zu) outside the %zu x %zu matrix\n", i, (size_t)ixA[i], (size_t)ixB[i], dimA, dimB);
            return nan;
        }
        hr[i] = (unsigned)ixA[i];
        hc[i] = (unsigned)ixB[i];
    }
    const int device = pmf_env_device();
    if (hipSetDevice(device) != hipSuccess) {
        fprintf(stderr, "eval_llk: no usable HIP device\n");
        return nan;
    }
    const hipStream_t st = nullptr;
    const size_t kk = (size_t)k;
    real_t *dA = nullptr, *dB = nullptr, *d_val = nullptr, *d_cval = nullptr;
    unsigned *d_row = nullptr, *d_col = nullptr, *d_minor = nullptr;
    unsigned long long* d_indptr = nullptr;
    double* d_scratch = nullptr;
    size_t uniq = 0;
    double out = 0.0;
    bool ok = false;
    do {
        if (pmf_alloc(&dA, dimA * kk * sizeof(real_t), st) != hipSuccess || pmf_alloc(&dB, dimB * kk * sizeof(real_t), st) != hipSuccess ||
            pmf_alloc(&d_indptr, (dimA + 1) * sizeof(unsigned long long), st) != hipSuccess)
            break;
        if (pmf_upload_big(dA, A, dimA * kk * sizeof(real_t), device, st) != hipSuccess || pmf_upload_big(dB, B, dimB * kk * sizeof(real_t), device, st) != hipSuccess)
            break;
        if (nnz > 0) {
            if (pmf_alloc(&d_row, nnz * sizeof(unsigned), st) != hipSuccess || pmf_alloc(&d_col, nnz * sizeof(unsigned), st) != hipSuccess ||
                pmf_alloc(&d_val, nnz * sizeof(real_t), st) != hipSuccess || pmf_alloc(&d_minor, nnz * sizeof(unsigned), st) != hipSuccess ||
                pmf_alloc(&d_cval, nnz * sizeof(real_t), st) != hipSuccess)
                break;
            if (pmf_upload(d_row, hr.data(), nnz * sizeof(unsigned), st) != hipSuccess ||
                pmf_upload(d_col, hc.data(), nnz * sizeof(unsigned), st) != hipSuccess || pmf_upload(d_val, X, nnz * sizeof(real_t), st) != hipSuccess)
                break;
            // duplicates summed, indices sorted: the CSR PoisMF.fit's session holds for the same triplets
            if (poismf_hip_device_coo_to_cs(d_row, d_col, d_val, nnz, 0, dimA, d_minor, d_cval, d_indptr, &uniq, st)) break;
        }
        if (pmf_alloc(&d_scratch, poismf_hip_llk_scratch(dimA, dimB, kk, uniq) * sizeof(double), st) != hipSuccess) break;
        if (poismf_hip_llk_enqueue(dA, dB, dimA, dimB, kk, d_indptr, d_minor, d_cval, uniq, full_llk, include_missing, d_scratch, st)) break;
        if (pmf_download(&out, d_scratch, sizeof(double), st) != hipSuccess) break;
        ok = true;
    } while (0);
    pmf_free(dA, st);
    pmf_free(dB, st);
    pmf_free(d_indptr, st);
    pmf_free(d_row, st);
    pmf_free(d_col, st);
    pmf_free(d_val, st);
    pmf_free(d_minor, st);
    pmf_free(d_cval, st);
    pmf_free(d_scratch, st);
    if (!ok) {
        const hipError_t e = hipGetLastError();
        fprintf(stderr, "eval_llk: device error or out of memory (%s)\n", hipGetErrorString(e));
        return nan;
    }
    return (long double)out;
}

}  // extern "C"
