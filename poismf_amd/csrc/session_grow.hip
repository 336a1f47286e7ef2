// session_grow.hip -- a resident session takes new rows (include/poismf_hip.h section 2d): users or items the model has never seen join
// it in place.  The growth itself -- the grown factor in its compact and its line-padded copy, the grown row pointers, the per-row
// counters of a profiling session -- is built beside the resident arrays and swapped in when all of it exists; the new rows' cells then go
// through section 2b's merge (session_merge.hpp: merge_half) as device triplets, for both orientations, and finish_half sorts and bins each
// half again.  adopt_new takes rows, cells and solved factors from the session's guest (fold_in.hip) without a trip to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "session_merge.hpp"

namespace {

// ---- the growth kernels -----------------------------------------------------------------------------------------------------------------

template <class T> struct alignas(16) Piece { T v[16 / sizeof(T)]; };

// The grown factor in one pass: rows [0, old_dim) from the old compact factor, rows [old_dim, new_dim) from F (nullptr: zeros), then the
// all-zero row and the 16 bytes of slack session_alloc promises behind a factor -- written to the compact copy `out` and, where the session
// keeps one (outp != nullptr, row stride ld), to the line-padded copy with its pad columns zero.  A lane holds one 16-byte piece of a
// row of ld elements (ld == k without a padded copy: k * sizeof(T) is then a multiple of 16), lanes on consecutive pieces: the padded
// side is always one aligned 16-byte store, the compact side a 16-byte load and store where its row starts on a 16-byte boundary (every
// row without a padded copy, every other row at k = 50 fp32) and element accesses otherwise.  Every byte of both allocations is written
// once and no old byte is read twice.
template <class T>
__global__ __launch_bounds__(256) void grow_factor_kernel(const T* __restrict__ old, const T* __restrict__ F, size_t old_dim, size_t new_dim, int k,
                                                          int ld, T* __restrict__ out, T* __restrict__ outp)
{
    constexpr int E = 16 / sizeof(T);
    const size_t P = (size_t)ld / E;               // pieces per row
    const size_t total = (new_dim + 1) * P + 1;    // rows, the zero row, one piece of slack
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / P;
        const int c0 = (int)(i - row * P) * E;
        const bool slack = row > new_dim;
        const int n = slack ? E : std::max(0, std::min(k - c0, E));   // elements of the piece that the compact copy holds
        const size_t at = row * (size_t)k + (size_t)c0;               // ... and where
        const T* src = nullptr;
        size_t from = 0;
        if (row < old_dim) { src = old; from = at; }
        else if (row < new_dim && F != nullptr) { src = F; from = (row - old_dim) * (size_t)k + (size_t)c0; }
        Piece<T> v;
#pragma unroll
        for (int j = 0; j < E; j++) v.v[j] = (T)0;
        if (src != nullptr) {
            if (n == E && from % E == 0) v = *reinterpret_cast<const Piece<T>*>(src + from);
            else {
#pragma unroll
                for (int j = 0; j < E; j++)
                    if (j < n) v.v[j] = src[from + j];
            }
        }
        if (n == E && at % E == 0) *reinterpret_cast<Piece<T>*>(out + at) = v;
        else {
#pragma unroll
            for (int j = 0; j < E; j++)
                if (j < n) out[at + j] = v.v[j];
        }
        if (outp != nullptr) *reinterpret_cast<Piece<T>*>(outp + row * (size_t)ld + (size_t)c0) = v;
    }
}

// the grown row pointers: the old ones, then nnz for every new (empty) row
__global__ __launch_bounds__(256) void grow_indptr_kernel(const u64* indptr, size_t old_dim, u64 nnz, size_t new_dim, u64* out)
{
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= new_dim; r += (size_t)gridDim.x * blockDim.x) out[r] = r <= old_dim ? indptr[r] : nnz;
}

// One lane per cell e of a CSR of n rows: its row is the last r with indptr[r] <= e; the cell's major index is first + r.
__global__ __launch_bounds__(256) void grow_major_kernel(const u64* indptr, size_t n, size_t total, unsigned first, unsigned* major)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        major[e] = first + (unsigned)upd_row_of(indptr, 0, n - 1, e);
    }
}

// ---- the growth step ----------------------------------------------------------------------------------------------------------------------

// n_new empty rows behind half `which` (1: users, 0: items), their factor rows from d_F (device [n_new x k], or nullptr: zeros).  All new
// arrays are built beside the old ones and take their place only when all exist: a failure (1) leaves the session as it was.  Afterwards
// the grown half has no permutation and no descriptors: the caller owes it a finish_half.
int grow(poismf_hip_session* s, int which, size_t n_new, const real_t* d_F)
{
    const hipStream_t st = s->stream;
    Half& h = s->half[which];
    const size_t k = s->k, old_dim = h.dimM, new_dim = old_dim + n_new;
    const size_t slack = 16 / sizeof(real_t);   // (the 16 bytes session_alloc promises behind a factor)
    real_t*& M = which ? s->dA : s->dB;
    real_t*& Mp = which ? s->dAp : s->dBp;
    Scratch sc(st);   // (what has not been handed to the session goes with it)
    real_t *new_M = nullptr, *new_Mp = nullptr;
    u64* new_indptr = nullptr;
    unsigned *eval_rows = nullptr, *dec_rows = nullptr;
    HIP_TRY(sc.get(&new_M, (new_dim + 1) * k + slack));
    if (s->ld != 0) HIP_TRY(sc.get(&new_Mp, (new_dim + 1) * s->ld + slack));
    HIP_TRY(sc.get(&new_indptr, new_dim + 1));
    if (h.d_eval_rows != nullptr) HIP_TRY(sc.get(&eval_rows, new_dim));
    if (h.d_dec_rows != nullptr) HIP_TRY(sc.get(&dec_rows, 2 * new_dim));
    {
        const size_t ld = s->ld != 0 ? s->ld : k;
        const size_t pieces = (new_dim + 1) * (ld * sizeof(real_t) / 16) + 1;
        const unsigned blocks = (unsigned)std::min<size_t>((pieces + 255) / 256, (size_t)s->num_cu * 16);
        hipLaunchKernelGGL((grow_factor_kernel<real_t>), dim3(blocks), dim3(256), 0, st, M, d_F, old_dim, new_dim, (int)k, (int)ld, new_M, new_Mp);
    }
    hipLaunchKernelGGL(grow_indptr_kernel, dim3(grid_for(new_dim + 1)), dim3(256), 0, st, h.d_indptr, old_dim, (u64)h.nnz, new_dim, new_indptr);
    HIP_TRY(hipGetLastError());
    // a profiling session's per-row counters: the old rows keep theirs, the new rows start at zero
    if (eval_rows != nullptr) {
        HIP_TRY(hipMemcpyAsync(eval_rows, h.d_eval_rows, sizeof(unsigned) * old_dim, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(eval_rows + old_dim, 0, sizeof(unsigned) * n_new, st));
    }
    if (dec_rows != nullptr) {
        HIP_TRY(hipMemcpyAsync(dec_rows, h.d_dec_rows, 2 * sizeof(unsigned) * old_dim, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(dec_rows + 2 * old_dim, 0, 2 * sizeof(unsigned) * n_new, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // the swap: from here on the session has the grown dimension
    if (s->partials_of == M) { s->partials_given = false; s->partials_of = nullptr; }   // partial sums of a factor that goes
    pmf_free(M, st); pmf_free(Mp, st); pmf_free(h.d_indptr, st);
    pmf_free(h.d_perm, st); pmf_free(h.d_desc, st);   // (finish_half sizes them anew)
    pmf_free(h.d_eval_rows, st); pmf_free(h.d_dec_rows, st);
    M = sc.release(new_M); Mp = sc.release(new_Mp); h.d_indptr = sc.release(new_indptr);
    h.d_eval_rows = sc.release(eval_rows); h.d_dec_rows = sc.release(dec_rows);
    h.d_perm = nullptr; h.d_desc = nullptr;
    // (the padded copy was built from the compact rows: it is as fresh as it was -- padded_fresh[which] stays)
    (which ? s->dimA : s->dimB) = new_dim;
    h.dimM = h.row_end = new_dim;
    s->half[which ? 0 : 1].dimF = new_dim;
    s->topn_indptr.clear();   // exclude_seen reads the grown CSR's pointers
    if (!which && s->guest != nullptr) {   // the guest borrows B: a stale pointer would be read by the next new-rows call
        poismf_hip_session* q = s->guest;
        q->dB = s->dB; q->dBp = s->dBp; q->dimB = new_dim;
        q->half[1].dimF = new_dim;
    }
    return 0;
}

// Growth, then the new rows' cells: n triplets on the device, d_new their new-row index (global) and d_other the index in the other
// dimension; touched_new: the new rows that hold a cell, ascending; touched_other as merge_half's `touched`.  Each half is finished with
// the segments it had.  0 or 1.
int grow_and_merge(poismf_hip_session* s, int which, size_t n_new, const real_t* d_F, const unsigned* d_new, const unsigned* d_other,
                   const real_t* d_val, size_t n, const std::vector<unsigned>& touched_new, const std::vector<unsigned>* touched_other)
{
    Half& g = s->half[which];
    const int nseg = (int)std::max<size_t>(g.segs.size(), 1);
    if (grow(s, which, n_new, d_F)) return 1;
    if (n == 0) return finish_half(g, s->stream, nseg);
    const int rc = both_halves(s, [&](int w, Half& h, bool* swapped) {
        const bool grown = w == which;
        size_t fresh = 0;
        const int r = merge_half(s, h, grown ? d_new : d_other, grown ? d_other : d_new, d_val, n, grown ? &touched_new : touched_other, &fresh);
        *swapped = r == 0;
        return r;
    });
    if (rc && g.d_perm == nullptr) (void)finish_half(g, s->stream, nseg);   // the grown half is owed one even when a merge fails: its rows stay empty
    return rc ? 1 : 0;
}

}  // namespace

extern "C" {

int poismf_hip_session_append_rows(poismf_hip_session* s, int which, size_t n_new, const real_t* F, const real_t* val, const sparse_ix* indptr,
                                   const sparse_ix* indices, size_t* first_row)
{
    if (s == nullptr) return 1;
    which = which ? 1 : 0;
    const size_t dim = which ? s->dimA : s->dimB, other = which ? s->dimB : s->dimA;
    if (first_row != nullptr) *first_row = dim;
    if (n_new == 0) return 0;
    if (n_new > 0x7fffffffull || dim + n_new > 0x7fffffffull) return 1;
    size_t n = 0, base = 0;
    if (indptr != nullptr) {
        if ((long long)indptr[0] < 0) return 3;
        for (size_t i = 0; i < n_new; i++)
            if (indptr[i + 1] < indptr[i]) return 3;
        base = (size_t)indptr[0];
        n = (size_t)indptr[n_new] - base;
        if (n > 0xffffffffull || (n > 0 && (val == nullptr || indices == nullptr))) return 1;
        for (size_t i = 0; i < n_new; i++)
            for (size_t p = (size_t)indptr[i]; p < (size_t)indptr[i + 1]; p++) {
                if ((long long)indices[p] < 0 || (size_t)indices[p] >= other) return 3;
                if (p > (size_t)indptr[i] && (size_t)indices[p - 1] >= (size_t)indices[p]) return 3;
            }
        for (size_t p = base; p < base + n; p++)
            if (!std::isfinite(val[p]) || !(val[p] > (real_t)0)) return 4;
    }
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (const int e = eligible(s)) return e;
    const hipStream_t st = s->stream;
    std::vector<unsigned> touched_new, touched_other, major, h32;
    try {
        if (n > 0) {
            touched_other = distinct_sorted(indices + base, n, other);
            major.resize(n);   // the cells' new-row index, from the row pointers
            for (size_t i = 0; i < n_new; i++) {
                if (indptr[i + 1] > indptr[i]) touched_new.push_back((unsigned)(dim + i));
                for (size_t p = (size_t)indptr[i]; p < (size_t)indptr[i + 1]; p++) major[p - base] = (unsigned)(dim + i);
            }
            h32.resize(n);
        }
    } catch (const std::bad_alloc&) { return 1; }
    Scratch sc(st);
    real_t *d_F = nullptr, *d_val = nullptr;
    unsigned *d_new = nullptr, *d_other = nullptr;
    if (F != nullptr) {
        HIP_TRY(sc.get(&d_F, n_new * s->k));
        HIP_TRY(pmf_upload_big(d_F, F, n_new * s->k * sizeof(real_t), s->device, st));
    }
    if (n > 0 && upload_cells(sc, major.data(), indices + base, val + base, n, h32, &d_new, &d_other, &d_val)) return 1;
    return grow_and_merge(s, which, n_new, d_F, d_new, d_other, d_val, n, touched_new, &touched_other);
}

int poismf_hip_session_adopt_new(poismf_hip_session* s, size_t* first_row, size_t* n_rows)
{
    if (s == nullptr) return 1;
    if (first_row != nullptr) *first_row = s->dimA;
    if (n_rows != nullptr) *n_rows = 0;
    poismf_hip_session* g = s->guest;
    if (g == nullptr || g->dimA == 0) return 5;
    const size_t n_new = g->dimA, dim = s->dimA;
    const Half& gh = g->half[1];
    const size_t n = gh.d_indptr != nullptr ? gh.nnz : 0;
    if (dim + n_new > 0x7fffffffull || n > 0xffffffffull) return 1;
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    if (n > 0) {
        const int asc = rows_ascending(g, 1);
        if (asc < 0) return 1;
        if (asc == 0) return 5;
        if (!gh.x_positive) return 4;
    }
    if (const int e = eligible(s)) return e;
    const hipStream_t st = s->stream;
    std::vector<unsigned> touched_new;
    Scratch sc(st);
    unsigned* d_new = nullptr;
    if (n > 0) {
        // the counts: the guest's row pointers say which new rows hold a cell; the cells themselves stay on the device
        std::vector<u64> ip;
        try {
            ip.resize(n_new + 1);
            HIP_TRY(pmf_download(ip.data(), gh.d_indptr, sizeof(u64) * (n_new + 1), st));
            for (size_t i = 0; i < n_new; i++)
                if (ip[i + 1] > ip[i]) touched_new.push_back((unsigned)(dim + i));
        } catch (const std::bad_alloc&) { return 1; }
        HIP_TRY(sc.get(&d_new, n));
        hipLaunchKernelGGL(grow_major_kernel, dim3(grid_for(n)), dim3(256), 0, st, gh.d_indptr, n_new, n, (unsigned)dim, d_new);
        HIP_TRY(hipGetLastError());
    }
    // the guest's factor rows, column indices and values are read where they are
    const int rc = grow_and_merge(s, 1, n_new, g->dA, d_new, gh.d_indices, gh.d_values, n, touched_new, nullptr);
    if (rc == 0 && n_rows != nullptr) *n_rows = n_new;
    return rc;
}

}  // extern "C"
