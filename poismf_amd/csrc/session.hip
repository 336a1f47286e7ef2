// session.hip -- the device-resident session (include/poismf_hip.h, section 2) and its life cycle: the stream cache, allocation, the
// upload and device-side set-up of a half of X (sort rows by length, row descriptors, length bins), create / destroy, factors in and out,
// the profiling and statistics read-outs, segments, and the session's wrappers around serving, the likelihood and the batched calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "session.hpp"
#include "cores.hpp"
#include "tb_batch.hpp"
#include "tb_deep.hpp"

// Streams are recycled across sessions: creating one costs 7.5 ms on this stack (scripts/probes/h2d_probe.hip) -- with two
// per run_poismf call that was most of the call's set-up time on config C2.  Idle streams wait here, per device.
static std::mutex g_stream_mutex;
static std::vector<hipStream_t> g_idle_streams[64];
static int cached_stream(int device, hipStream_t* out)
{
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> lk(g_stream_mutex);
        auto& v = g_idle_streams[device];
        if (!v.empty()) { *out = v.back(); v.pop_back(); return 0; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking) != hipSuccess;
}
static void release_stream(int device, hipStream_t st)
{
    (void)hipStreamSynchronize(st);
    if (device >= 0 && device < 64) {
        std::lock_guard<std::mutex> lk(g_stream_mutex);
        if (g_idle_streams[device].size() < 8) { g_idle_streams[device].push_back(st); return; }
    }
    (void)hipStreamDestroy(st);
}

void free_half(Half& h, hipStream_t stream)
{
    pmf_free(h.d_indptr, stream);
    pmf_free(h.d_indices, stream);
    pmf_free(h.d_values, stream);
    pmf_free(h.d_perm, stream);
    pmf_free(h.d_desc, stream);
    pmf_free(h.d_eval_rows, stream);
    pmf_free(h.d_dec_rows, stream);
    h = Half();
}

namespace {

// ---- device-side set-up of one half ---------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rebase_indptr_kernel(unsigned long long* indptr, size_t n, unsigned long long base)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) indptr[i] -= base;
}

// flag |= 1 when some stored value is not > 0 (zero, negative, NaN)
__global__ __launch_bounds__(256) void values_positive_kernel(const real_t* v, size_t n, unsigned* flag)
{
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) bad = bad || !(v[i] > (real_t)0);
    if (bad) atomicOr(flag, 1u);
}
__global__ __launch_bounds__(256) void row_desc_kernel(const unsigned long long* indptr, const unsigned* perm, size_t n, RowDesc* desc)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned r = perm[i];
        const unsigned long long p0 = indptr[r];
        desc[i] = { (unsigned)p0, (unsigned)(p0 >> 32), (unsigned)(indptr[r + 1] - p0), r };
    }
}

}  // namespace

// h.d_indptr (shard-local, nloc + 1), h.d_indices, h.d_values are on the device: per segment, sort the rows by length
// (longest first, equal lengths in row order), build the row descriptors on the device and the length bins on the host
// (from the sorted lengths: 4 bytes per row come back over PCIe, the only host work left is one linear scan).
// In two steps, so that a caller can put other work (run_poismf: the factors' upload) between the launches and the one place that
// waits for them.
static int finish_half_launch(Half& h, hipStream_t stream, HalfPending& pend, int nseg = 1)
{
    const size_t nloc = h.row_end - h.row_begin;
    if (h.d_perm == nullptr) HIP_TRY(pmf_alloc(&h.d_perm, sizeof(unsigned) * (nloc ? nloc : 1), stream));
    if (h.d_desc == nullptr) HIP_TRY(pmf_alloc(&h.d_desc, sizeof(RowDesc) * (nloc ? nloc : 1), stream));
    h.segs.clear();
    nseg = std::max(nseg, 1);   // as asked (segments of a short shard may be empty): every rank cuts its shard the same way
    if (nloc == 0) { for (int j = 0; j < nseg; j++) h.segs.push_back({ 0u, 0u, {} }); return 0; }
    HIP_TRY(pmf_alloc(&pend.d_len, sizeof(unsigned) * nloc, stream));
    for (int j = 0; j < nseg; j++) {
        const size_t lo = segment_cut(nloc, j, nseg), hi = segment_cut(nloc, j + 1, nseg);
        h.segs.push_back({ (unsigned)lo, (unsigned)hi, {} });
        if (hi > lo && poismf_hip_device_sort_rows(h.d_indptr + lo, hi - lo, (unsigned)lo, h.d_perm + lo, pend.d_len + lo, stream)) {
            pmf_free(pend.d_len, stream);
            pend.d_len = nullptr;
            return 1;
        }
    }
    const unsigned grid = (unsigned)std::min<size_t>((nloc + 255) / 256, 2048);
    hipLaunchKernelGGL(row_desc_kernel, dim3(grid), dim3(256), 0, stream, h.d_indptr, h.d_perm, nloc, h.d_desc);
    // are all stored values positive (Poisson counts)?  One pass over the values, the flag rides in front of the lengths
    HIP_TRY(pmf_alloc(&pend.d_flag, sizeof(unsigned), stream));
    HIP_TRY(hipMemsetAsync(pend.d_flag, 0, sizeof(unsigned), stream));
    if (h.nnz > 0)
        hipLaunchKernelGGL(values_positive_kernel, dim3((unsigned)std::min<size_t>((h.nnz + 255) / 256, 2048)), dim3(256), 0, stream, h.d_values, h.nnz, pend.d_flag);
    return 0;
}
int finish_half_collect(Half& h, hipStream_t stream, HalfPending& pend)
{
    const size_t nloc = h.row_end - h.row_begin;
    if (nloc == 0) return 0;
    std::vector<unsigned> len(nloc);
    hipError_t e = pmf_download(len.data(), pend.d_len, sizeof(unsigned) * nloc, stream);
    unsigned not_positive = 1;
    if (e == hipSuccess) e = pmf_download(&not_positive, pend.d_flag, sizeof(unsigned), stream);
    h.x_positive = not_positive == 0;
    pmf_free(pend.d_flag, stream);
    pmf_free(pend.d_len, stream);
    pend = HalfPending();
    HIP_TRY(e);
    for (auto& sg : h.segs) sg.bins = bins_of(len.data(), sg.row_lo, sg.row_hi);
    return 0;
}
int finish_half(Half& h, hipStream_t stream, int nseg)
{
    HalfPending pend;
    if (finish_half_launch(h, stream, pend, nseg)) { pmf_free(pend.d_flag, stream); pmf_free(pend.d_len, stream); return 1; }
    return finish_half_collect(h, stream, pend);
}

// descriptors of the n rows d_perm names, in its order (a listed-rows half-sweep builds its own: session_update.hip)
int row_desc_launch(const unsigned long long* d_indptr, const unsigned* d_perm, size_t n, RowDesc* d_desc, hipStream_t stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(row_desc_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, stream, d_indptr, d_perm, n, d_desc);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Upload rows [r0, r1) of a host CSR (size_t indices) with shard-local pointers; the indices are narrowed to u32 on
// the device (the binding rejects dimensions above INT_MAX, ref: poismf_c_wrapper.pxi:78-80).
// (pend != nullptr: the row sort is launched but not waited for -- the caller owes a finish_half_collect)
int build_half(Half& h, hipStream_t stream, const real_t* val, const sparse_ix* indptr, const sparse_ix* indices,
               size_t dimM, size_t dimF, size_t r0, size_t r1, int device, HalfPending* pend)
{
    h.dimM = dimM; h.dimF = dimF; h.row_begin = r0; h.row_end = r1;
    const size_t nloc = r1 - r0;
    const size_t base = (size_t)indptr[r0];
    h.nnz = (size_t)indptr[r1] - base;
    HIP_TRY(pmf_alloc(&h.d_indptr, sizeof(unsigned long long) * (nloc + 1), stream));
    HIP_TRY(pmf_alloc(&h.d_indices, sizeof(unsigned) * (h.nnz ? h.nnz : 1), stream));
    HIP_TRY(pmf_alloc(&h.d_values, sizeof(real_t) * (h.nnz ? h.nnz : 1), stream));
    pmf_tl("half: device arrays allocated");
    if constexpr (sizeof(sparse_ix) == sizeof(unsigned long long)) {
        // C / Python ABI: size_t indices go up as they are and are narrowed to u32 by a kernel
        HIP_TRY(pmf_upload(h.d_indptr, indptr + r0, sizeof(unsigned long long) * (nloc + 1), stream));
        // indices: narrowed to u32 by host threads on their way into pinned chunks (half the bytes over PCIe, devmem.hpp); the
        // plain path -- whole size_t array up, narrowed by a kernel -- when the staged one is not available
        hipError_t se = hipErrorNotReady;
        if (h.nnz) {
            const sparse_ix* src = indices + base;
            se = pmf_upload_staged(h.d_indices, h.nnz, sizeof(unsigned), device, stream, [src](void* pin, size_t i0, size_t cnt) {
                unsigned* o = (unsigned*)pin;
                const sparse_ix* q = src + i0;
                for (size_t i = 0; i < cnt; i++) o[i] = (unsigned)q[i];
            });
            if (se != hipSuccess && se != hipErrorNotReady) HIP_TRY(se);
            pmf_tl("half: row pointers up, indices narrowed and handed to the DMA queue");
        }
        if (h.nnz && se != hipSuccess) {
            unsigned long long* d_wide = nullptr;
            HIP_TRY(pmf_alloc(&d_wide, sizeof(unsigned long long) * h.nnz, stream));
            hipError_t e = pmf_upload(d_wide, indices + base, sizeof(unsigned long long) * h.nnz, stream);
            if (e == hipSuccess && poismf_hip_device_narrow(d_wide, h.nnz, h.d_indices, stream)) e = hipErrorUnknown;
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            pmf_free(d_wide, stream);
            HIP_TRY(e);
        }
    } else {
        // R ABI: int indices are the device's width already; the row pointers are widened on the host (dim + 1 values)
        std::vector<unsigned long long> wide(nloc + 1);
        for (size_t i = 0; i <= nloc; i++) wide[i] = (unsigned long long)indptr[r0 + i];
        HIP_TRY(pmf_upload(h.d_indptr, wide.data(), sizeof(unsigned long long) * (nloc + 1), stream));
        HIP_TRY(pmf_upload(h.d_indices, indices + base, sizeof(unsigned) * h.nnz, stream));
    }
    if (base != 0) {
        hipLaunchKernelGGL(rebase_indptr_kernel, dim3((unsigned)std::min<size_t>((nloc + 256) / 256, 2048)), dim3(256), 0, stream, h.d_indptr, nloc + 1,
                           (unsigned long long)base);
    }
    {
        const real_t* src = val + base;
        const hipError_t se = pmf_upload_staged(h.d_values, h.nnz, sizeof(real_t), device, stream, [src](void* pin, size_t i0, size_t cnt) {
            memcpy(pin, src + i0, cnt * sizeof(real_t));
        });
        if (se == hipErrorNotReady) HIP_TRY(pmf_upload(h.d_values, val + base, sizeof(real_t) * h.nnz, stream));
        else HIP_TRY(se);
    }
    pmf_tl("half: values handed to the DMA queue");
    if (pend != nullptr) {
        if (finish_half_launch(h, stream, *pend)) { pmf_free(pend->d_flag, stream); pmf_free(pend->d_len, stream); *pend = HalfPending(); return 1; }
        return 0;
    }
    const int bad = finish_half(h, stream);
    pmf_tl("half: rows sorted, lengths back, bins cut");
    return bad;
}

// Everything of a session except the two halves of X: streams, the replicated factors (+ their line-padded gather
// copies), column-sum scratch.  On failure the partly built session is destroyed and nullptr returned.
poismf_hip_session* session_alloc(int device, void* stream, size_t dimA, size_t dimB, size_t k)
{
    if (k == 0 || slots_per_lane(k) == 0 || nc_for_k(k) == 0) {
        fprintf(stderr, "poismf_hip: k = %zu is outside the supported range (1..%d)\n", k, 128 * SLOT_ELEMS);
        return nullptr;
    }
    if (const hipError_t e = hipSetDevice(device); e != hipSuccess) {   // no device, wrong index: rc 1, and stderr says it was not memory
        pmf_last_hip_error() = e;
        return nullptr;
    }
    poismf_hip_session* s = new (std::nothrow) poismf_hip_session();
    if (!s) return nullptr;
    s->device = device;
    {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) s->num_cu = n;
    }
    {
        int khz = 0;   // constant-rate counter behind wall_clock64(): 100 MHz on this part
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) s->gate_budget = 2ull * (unsigned long long)khz;
    }
    s->stream = (hipStream_t)stream;
    auto fail = [&]() -> poismf_hip_session* { poismf_hip_session_destroy(s); return nullptr; };
    if (s->stream == nullptr) {  // no stream given: the session owns a non-blocking stream (NOT the legacy default stream)
        if (cached_stream(device, &s->stream)) { delete s; return nullptr; }
        s->owns_stream = true;
    }
    s->dimA = dimA; s->dimB = dimB; s->k = k;
    // behind each factor: one all-zero row (the register engine points the unused steps of a row at it) + 16 B so that
    // the last 16-byte slot of the last row stays in bounds
    const size_t slack = k * sizeof(real_t) + 16;
    if (pmf_alloc(&s->dA, dimA * k * sizeof(real_t) + slack, s->stream) != hipSuccess) return fail();
    if (pmf_alloc(&s->dB, dimB * k * sizeof(real_t) + slack, s->stream) != hipSuccess) return fail();
    if (hipMemsetAsync(s->dA, 0, dimA * k * sizeof(real_t) + slack, s->stream) != hipSuccess) return fail();
    if (hipMemsetAsync(s->dB, 0, dimB * k * sizeof(real_t) + slack, s->stream) != hipSuccess) return fail();
    {
        // A gathered row of B bytes at an arbitrary 8-byte offset touches (B + 120) / 128 lines of 128 bytes on average;
        // in a copy whose rows start on line boundaries it touches ceil(B / 128).  k = 50 fp32: 2.5 -> 2 lines.
        const size_t rowb = k * sizeof(real_t), padb = padded_row_bytes(k);
        if (padb != rowb) {
            s->ld = padb / sizeof(real_t);
            const size_t pslack = padb + 16;
            if (pmf_alloc(&s->dAp, dimA * padb + pslack, s->stream) != hipSuccess) return fail();
            if (pmf_alloc(&s->dBp, dimB * padb + pslack, s->stream) != hipSuccess) return fail();
            if (hipMemsetAsync(s->dAp, 0, dimA * padb + pslack, s->stream) != hipSuccess) return fail();
            if (hipMemsetAsync(s->dBp, 0, dimB * padb + pslack, s->stream) != hipSuccess) return fail();
        }
    }
    if (pmf_alloc(&s->d_bsum, k * sizeof(real_t) + slack, s->stream) != hipSuccess) return fail();
    if (pmf_alloc(&s->d_partial, (size_t)s->colsum_waves * k * sizeof(real_t), s->stream) != hipSuccess) return fail();
    if (pmf_alloc(&s->d_counter, sizeof(unsigned), s->stream) != hipSuccess) return fail();
    if (pmf_alloc(&s->d_queue, sizeof(unsigned) * (MAX_LAUNCHES + 2 * TEAM_LAUNCH_MAX), s->stream) != hipSuccess) return fail();   // (+: a head of its own for every team launch of a half, and one for its streamed re-run)
    if (pmf_alloc(&s->d_arrive, sizeof(unsigned), s->stream) != hipSuccess) return fail();
    if (pmf_alloc(&s->d_team_err, TEAM_ERR_WORDS * sizeof(unsigned), s->stream) != hipSuccess) return fail();
    if (hipMemsetAsync(s->d_team_err, 0, TEAM_ERR_WORDS * sizeof(unsigned), s->stream) != hipSuccess) return fail();
    if (cached_stream(device, &s->aux_stream)) return fail();
    if (hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess) return fail();
    if (hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) return fail();
    return s;
}

// One orientation of a device COO -> the half's own (exactly sized) CSR arrays, rows [m0, m1) only.
static int half_from_device_coo(Half& h, hipStream_t stream, const unsigned* d_major, const unsigned* d_minor, const real_t* d_val, size_t n,
                                size_t dimM, size_t dimF, size_t m0, size_t m1)
{
    h.dimM = dimM; h.dimF = dimF; h.row_begin = m0; h.row_end = m1;
    const size_t nloc = m1 - m0;
    unsigned* t_idx = nullptr;
    real_t* t_val = nullptr;
    HIP_TRY(pmf_alloc(&h.d_indptr, sizeof(unsigned long long) * (nloc + 1), stream));
    hipError_t e = pmf_alloc(&t_idx, sizeof(unsigned) * n, stream);
    if (e == hipSuccess) e = pmf_alloc(&t_val, sizeof(real_t) * n, stream);
    size_t uniq = 0;
    int rc = e != hipSuccess;
    if (!rc) rc = poismf_hip_device_coo_to_cs(d_major, d_minor, d_val, n, m0, m1, t_idx, t_val, h.d_indptr, &uniq, stream);
    if (!rc) {
        h.nnz = uniq;
        // the conversion's outputs have room for all n triplets; the session keeps exactly sized copies
        if (pmf_alloc(&h.d_indices, sizeof(unsigned) * (uniq ? uniq : 1), stream) != hipSuccess ||
            pmf_alloc(&h.d_values, sizeof(real_t) * (uniq ? uniq : 1), stream) != hipSuccess ||
            hipMemcpyAsync(h.d_indices, t_idx, sizeof(unsigned) * uniq, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(h.d_values, t_val, sizeof(real_t) * uniq, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            rc = 1;
    }
    pmf_free(t_idx, stream);
    pmf_free(t_val, stream);
    return rc ? 1 : finish_half(h, stream);
}

// exclude_seen of the two batched calls below: the session's resident CSR shard as their exclusion lists; false when a user lies outside it
static bool session_seen(poismf_hip_session* s, const sparse_ix* users, size_t n_users, PmfTopnSeen& seen)
{
    const Half& h = s->half[1];
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] < h.row_begin || (size_t)users[i] >= h.row_end) return false;
    seen = { h.d_indptr, h.d_indices, h.row_begin, h.row_end, &s->topn_indptr, &s->csr_rows_sorted };
    return true;
}

extern "C" {

int poismf_hip_session_create(poismf_hip_session** out, int device, void* stream, const real_t* Xr,
                              const sparse_ix* Xr_indptr, const sparse_ix* Xr_indices, const real_t* Xc,
                              const sparse_ix* Xc_indptr, const sparse_ix* Xc_indices, size_t dimA, size_t dimB, size_t k,
                              size_t rowA_begin, size_t rowA_end, size_t rowB_begin, size_t rowB_end)
{
    *out = nullptr;
    if (rowA_end > dimA || rowB_end > dimB || rowA_begin > rowA_end || rowB_begin > rowB_end) return 1;
    poismf_hip_session* s = session_alloc(device, stream, dimA, dimB, k);
    if (!s) return 1;
    auto fail = [&]() { poismf_hip_session_destroy(s); return 1; };
    // half 0 updates B: rows of the CSC; half 1 updates A: rows of the CSR
    if (Xc_indptr != nullptr &&
        build_half(s->half[0], s->stream, Xc, Xc_indptr, Xc_indices, dimB, dimA, rowB_begin, rowB_end, device)) return fail();
    if (build_half(s->half[1], s->stream, Xr, Xr_indptr, Xr_indices, dimA, dimB, rowA_begin, rowA_end, device)) return fail();
    *out = s;
    return 0;
}

int poismf_hip_session_create_coo(poismf_hip_session** out, int device, void* stream, const sparse_ix* row, const sparse_ix* col,
                                  const real_t* val, size_t n, size_t dimA, size_t dimB, size_t k, size_t rowA_begin,
                                  size_t rowA_end, size_t rowB_begin, size_t rowB_end)
{
    *out = nullptr;
    if (n == 0 || n > 0xffffffffull || dimA > 0x7fffffffull || dimB > 0x7fffffffull) return 1;
    if (rowA_end > dimA || rowB_end > dimB || rowA_begin > rowA_end || rowB_begin > rowB_end) return 1;
    poismf_hip_session* s = session_alloc(device, stream, dimA, dimB, k);
    if (!s) return 1;
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    int rc = 1;
    do {
        if (pmf_alloc(&d_row, sizeof(unsigned) * n, s->stream) != hipSuccess || pmf_alloc(&d_col, sizeof(unsigned) * n, s->stream) != hipSuccess ||
            pmf_alloc(&d_val, sizeof(real_t) * n, s->stream) != hipSuccess)
            break;
        {
            std::vector<unsigned> h32;
            try { h32.resize(n); } catch (const std::bad_alloc&) { break; }
            // (an index outside the matrix -- or a negative one reinterpreted as size_t -- would become a gather offset into the
            // factors: rc 3, which the binding turns into ValueError)
            bool bad_index = false;
            for (size_t i = 0; i < n; i++) { bad_index |= (size_t)row[i] >= dimA; h32[i] = (unsigned)row[i]; }
            if (bad_index) { rc = 3; break; }
            if (hipMemcpy(d_row, h32.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice) != hipSuccess) break;
            for (size_t i = 0; i < n; i++) { bad_index |= (size_t)col[i] >= dimB; h32[i] = (unsigned)col[i]; }
            if (bad_index) { rc = 3; break; }
            if (hipMemcpy(d_col, h32.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice) != hipSuccess) break;
        }
        if (hipMemcpy(d_val, val, sizeof(real_t) * n, hipMemcpyHostToDevice) != hipSuccess) break;
        // half 0 updates B: the CSC (major = column); half 1 updates A: the CSR (major = row)
        if (half_from_device_coo(s->half[0], s->stream, d_col, d_row, d_val, n, dimB, dimA, rowB_begin, rowB_end)) break;
        if (half_from_device_coo(s->half[1], s->stream, d_row, d_col, d_val, n, dimA, dimB, rowA_begin, rowA_end)) break;
        rc = 0;
    } while (0);
    pmf_free(d_row, s->stream);
    pmf_free(d_col, s->stream);
    pmf_free(d_val, s->stream);
    if (rc) { poismf_hip_session_destroy(s); return rc; }
    *out = s;
    return 0;
}

void poismf_hip_session_destroy(poismf_hip_session* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->guest != nullptr) { poismf_hip_session_destroy(s->guest); s->guest = nullptr; }   // (before anything the guest borrows goes)
    if (s->borrows_B) {   // a guest (fold_in.hip): B, its padded copy, the streams and the events are its host's
        s->dB = s->dBp = nullptr;
        s->aux_stream = nullptr; s->owns_stream = false;
        s->ev_fork = s->ev_join = nullptr;
    }
    (void)hipStreamSynchronize(s->stream);
    if (s->aux_stream) (void)hipStreamSynchronize(s->aux_stream);
    for (auto& p : s->prof) { (void)hipEventDestroy(p.t0); (void)hipEventDestroy(p.t1); }
    s->prof.clear();
    for (auto& p : s->lprof) { (void)hipEventDestroy(p.t0); (void)hipEventDestroy(p.t1); }
    s->lprof.clear();
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    const hipStream_t own = s->owns_stream ? s->stream : nullptr, aux = s->aux_stream;
    free_half(s->half[0], s->stream);
    free_half(s->half[1], s->stream);
    pmf_free(s->dA, s->stream);
    pmf_free(s->dB, s->stream);
    pmf_free(s->dAp, s->stream);
    pmf_free(s->dBp, s->stream);
    pmf_free(s->d_bsum, s->stream);
    pmf_free(s->d_partial, s->stream);
    pmf_free(s->d_counter, s->stream);
    pmf_free(s->d_queue, s->stream);
    pmf_free(s->d_gt, s->stream);
    pmf_free(s->d_team, s->stream);
    pmf_free(s->d_team_err, s->stream);
    pmf_free(s->d_arrive, s->stream);
    pmf_free(s->d_team_backup, s->stream);
    pmf_free(s->d_team_eval_backup, s->stream);
    pmf_free(s->d_llk, s->stream);
    pmf_free(s->d_topn, s->stream);
    (void)hipStreamSynchronize(s->stream);   // the stream-ordered frees have run
    if (aux) release_stream(s->device, aux);
    if (own) release_stream(s->device, own);
    delete s;
}

// the device arrays kept from finished sessions (devmem.hpp) go back to the driver
void poismf_hip_release_cache(void) { pmf_release_cache(); }
// how much released device memory may be kept for the next call (MB; 0 = nothing, the default); returns the previous limit
size_t poismf_hip_set_device_cache_mb(size_t mb) { return pmf_set_cache_limit_mb(mb); }

// Whoever asks for the device pointers may write through them: the padded gather copies are re-derived afterwards.
real_t* poismf_hip_session_A(poismf_hip_session* s) { s->padded_fresh[1] = false; return s->dA; }
real_t* poismf_hip_session_B(poismf_hip_session* s) { s->padded_fresh[0] = false; return s->dB; }
// ... and whoever keeps such a pointer says so after every later write (which = 0: B was written, 1: A)
void poismf_hip_session_factors_dirty(poismf_hip_session* s, int which)
{
    s->padded_fresh[which ? 1 : 0] = false;
    if (s->partials_of == (which ? s->dA : s->dB)) { s->partials_given = false; s->partials_of = nullptr; }   // partial sums of a factor written since
}

void* poismf_hip_session_stream(poismf_hip_session* s) { return (void*)s->stream; }
size_t poismf_hip_session_nnz(poismf_hip_session* s, int which) { return s->half[which ? 1 : 0].nnz; }

int poismf_hip_session_set_factors(poismf_hip_session* s, const real_t* A_host, const real_t* B_host)
{
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(pmf_upload_big(s->dA, A_host, s->dimA * s->k * sizeof(real_t), s->device, s->stream));
    HIP_TRY(pmf_upload_big(s->dB, B_host, s->dimB * s->k * sizeof(real_t), s->device, s->stream));
    s->padded_fresh[0] = s->padded_fresh[1] = false;
    s->partials_given = false; s->partials_of = nullptr;
    return 0;
}

int poismf_hip_session_get_factors(poismf_hip_session* s, real_t* A_host, real_t* B_host)
{
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(pmf_download_big(A_host, s->dA, s->dimA * s->k * sizeof(real_t), s->device, s->stream));
    HIP_TRY(pmf_download_big(B_host, s->dB, s->dimB * s->k * sizeof(real_t), s->device, s->stream));
    return team_check(s);
}

void poismf_hip_session_profile(poismf_hip_session* s, int enable)
{
    (void)hipStreamSynchronize(s->stream);
    for (auto& p : s->prof) { (void)hipEventDestroy(p.t0); (void)hipEventDestroy(p.t1); }
    s->prof.clear();
    for (auto& p : s->lprof) { (void)hipEventDestroy(p.t0); (void)hipEventDestroy(p.t1); }
    s->lprof.clear();
    s->profiling = enable != 0;
    for (Half& h : s->half) {
        const size_t n = h.row_end - h.row_begin;
        if (s->profiling && h.d_eval_rows == nullptr && n > 0 && pmf_alloc(&h.d_eval_rows, sizeof(unsigned) * n, s->stream) != hipSuccess) h.d_eval_rows = nullptr;
        if (h.d_eval_rows != nullptr) (void)hipMemsetAsync(h.d_eval_rows, 0, sizeof(unsigned) * n, s->stream);
        if (s->profiling && h.d_dec_rows == nullptr && n > 0 && pmf_alloc(&h.d_dec_rows, 2 * sizeof(unsigned) * n, s->stream) != hipSuccess) h.d_dec_rows = nullptr;
        if (h.d_dec_rows != nullptr) (void)hipMemsetAsync(h.d_dec_rows, 0, 2 * sizeof(unsigned) * n, s->stream);
    }
}

int poismf_hip_session_kernel_time(poismf_hip_session* s, int which, double* total_ms, size_t* launches)
{
    HIP_TRY(hipStreamSynchronize(s->stream));
    double tot = 0;
    size_t n = 0;
    for (auto& p : s->prof) {
        if (p.which != which) continue;
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.t0, p.t1));
        tot += ms;
        n++;
    }
    *total_ms = tot;
    *launches = n;
    return 0;
}

int poismf_hip_session_eval_stats(poismf_hip_session* s, int which, unsigned long long* tile_passes, unsigned long long* nnz_passes)
{
    HIP_TRY(hipStreamSynchronize(s->stream));
    Half& h = s->half[which ? 1 : 0];
    const size_t n = h.row_end - h.row_begin;
    *tile_passes = 0;
    *nnz_passes = 0;
    if (h.d_eval_rows == nullptr || n == 0) return 0;
    std::vector<unsigned> ev(n);
    std::vector<unsigned long long> ptr(n + 1);
    HIP_TRY(hipMemcpy(ev.data(), h.d_eval_rows, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ptr.data(), h.d_indptr, sizeof(unsigned long long) * (n + 1), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        *tile_passes += ev[i];
        *nnz_passes += (unsigned long long)ev[i] * (ptr[i + 1] - ptr[i]);
    }
    return 0;
}

// The decisions of the solver on every row of half `which` in the most recent half-sweep of a profiling session: out[2 r] =
// iterations | rc << 24, out[2 r + 1] = evaluations, counted as the reference's minimize_nonneg_cg / tnc count them (local row r).
int poismf_hip_session_decisions(poismf_hip_session* s, int which, unsigned* out, size_t nrows)
{
    Half& h = s->half[which ? 1 : 0];
    if (h.d_dec_rows == nullptr) return 1;
    HIP_TRY(pmf_download(out, h.d_dec_rows, 2 * sizeof(unsigned) * std::min(nrows, h.row_end - h.row_begin), s->stream));
    return 0;
}

// Sums over the rows of half `which` of what the solvers decided in the most recent half-sweep of a profiling session, for the
// flop count the reference's arithmetic would need for the same decisions ("Flops"): out[0] = sum of iterations,
// out[1] = sum of evaluations, out[2] = sum of nnz x iterations, out[3] = sum of nnz x evaluations.
int poismf_hip_session_decision_stats(poismf_hip_session* s, int which, unsigned long long* out)
{
    HIP_TRY(hipStreamSynchronize(s->stream));
    Half& h = s->half[which ? 1 : 0];
    const size_t n = h.row_end - h.row_begin;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (h.d_dec_rows == nullptr) return 1;
    if (n == 0) return 0;
    std::vector<unsigned> dec(2 * n);
    std::vector<unsigned long long> ptr(n + 1);
    HIP_TRY(hipMemcpy(dec.data(), h.d_dec_rows, 2 * sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ptr.data(), h.d_indptr, sizeof(unsigned long long) * (n + 1), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        const unsigned long long it = dec[2 * i] & 0xffffffu, ev = dec[2 * i + 1], nz = ptr[i + 1] - ptr[i];
        out[0] += it; out[1] += ev; out[2] += nz * it; out[3] += nz * ev;
    }
    return 0;
}

// Serving from the session's resident factors: predict_multiple (ref: src/pred.c:42-64) and topN for the
// user in row `user` of A (ref: src/topN.c:112-284) without copying the factors per call.
int poismf_hip_session_predict(poismf_hip_session* s, const sparse_ix* ixA, const sparse_ix* ixB, size_t n, real_t* out)
{
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++)
        if ((size_t)ixA[i] >= s->dimA || (size_t)ixB[i] >= s->dimB) return 2;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return poismf_hip_serve_predict(s->dA, s->dB, ixA, ixB, n, (int)s->k, out, nullptr, nullptr);
}

// Poisson log-likelihood of the resident CSR shard under the resident (compact) factors -- the padded gather copies play no part,
// so no write through the factor pointers can leave a stale value behind.  Ordered after everything enqueued on the session stream.
int poismf_hip_session_llk(poismf_hip_session* s, int full_llk, int include_missing, double* out)
{
    HIP_TRY(hipSetDevice(s->device));
    const Half& h = s->half[1];
    const size_t nrows = h.row_end - h.row_begin;
    const size_t need = poismf_hip_llk_scratch(nrows, s->dimB, s->k, h.nnz);
    HIP_TRY(grow_buffer(s->d_llk, s->llk_cap, need, sizeof(double), s->stream));
    if (poismf_hip_llk_enqueue(s->dA + h.row_begin * s->k, s->dB, nrows, s->dimB, s->k, h.d_indptr, h.d_indices, h.d_values, h.nnz,
                               full_llk, include_missing, s->d_llk, s->stream))
        return 1;
    HIP_TRY(pmf_download(out, s->d_llk, sizeof(double), s->stream));
    return 0;
}

int poismf_hip_session_topn(poismf_hip_session* s, size_t user, const sparse_ix* include_ix, size_t n_include, const sparse_ix* exclude_ix,
                            size_t n_exclude, sparse_ix* outp_ix, real_t* outp_score, size_t n_top)
{
    if (user >= s->dimA) return 2;
    if (const int rc = poismf_hip_serve_topn_check(include_ix, n_include, exclude_ix, n_exclude, n_top, s->dimB)) return rc;
    for (size_t i = 0; include_ix && i < n_include; i++)
        if ((size_t)include_ix[i] >= s->dimB) return 2;
    for (size_t i = 0; exclude_ix && i < n_exclude; i++)
        if ((size_t)exclude_ix[i] >= s->dimB) return 2;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return poismf_hip_serve_topn(s->dA + user * s->k, s->dB, (int)s->k, include_ix, n_include, exclude_ix, n_exclude, outp_ix, outp_score,
                                 n_top, s->dimB);
}

// Batched top-N from the resident (compact) factors (topn_batch.hip; include/poismf_hip.h section 1f).  Ordered after the work already
// enqueued on the session stream; with exclude_seen the resident CSR shard's rows are the exclusion lists -- nothing of them is uploaded.
int poismf_hip_session_topn_batch(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, int exclude_seen,
                                  const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_batch_check(users, n_users, n_top, s->dimA, s->dimB, s->k, excl_indptr, excl_indices)) return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_batch_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, exclude_seen ? &seen : nullptr,
                                     excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Deep batched top-N from the resident (compact) factors (topn_deep.hip; include/poismf_hip.h section 1l), ordered as the call above and
// in the same scratch, which it may grow: a short row is padded, so nothing is counted beforehand.
int poismf_hip_session_topn_deep(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, int exclude_seen,
                                 const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_deep_check(users, n_users, n_top, s->dimA, s->dimB, s->k, excl_indptr, excl_indices)) return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_deep_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, exclude_seen ? &seen : nullptr,
                                    excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Batched top-N with per-group quotas from the resident (compact) factors (topn_quota.hip; include/poismf_hip.h section 1n), ordered as
// the calls above and in the same scratch: a short row is padded, so nothing is counted beforehand.
int poismf_hip_session_topn_quota(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* group_of,
                                  size_t n_groups, const sparse_ix* quota, int exclude_seen, const sparse_ix* excl_indptr,
                                  const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_quota_check(users, n_users, n_top, s->dimA, s->dimB, s->k, group_of, n_groups, quota, excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_quota_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, group_of, n_groups, quota,
                                     exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Batched top-N with per-item score weights from the resident (compact) factors (topn_weighted.hip; include/poismf_hip.h section 1o),
// ordered as the calls above and in the same scratch.  query_B: `users` are rows of the resident B -- the queries of an item-to-item
// call -- so B is both factor arguments of the core; the CSR shard has no rows for them, hence no exclude_seen.
int poismf_hip_session_topn_weighted(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, const real_t* item_weight,
                                     int query_B, int exclude_seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                     sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (query_B && exclude_seen) return 2;
    if (const int rc = poismf_hip_topn_weighted_check(users, n_users, n_top, query_B ? s->dimB : s->dimA, s->dimB, s->k, item_weight, excl_indptr,
                                                      excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_weighted_run(s->stream, query_B ? s->dB : s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, item_weight,
                                        exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Batched top-N with per-(user, item) score factors from the resident (compact) factors (topn_adjust.hip; include/poismf_hip.h section
// 1r), ordered as the calls above and in the same scratch.
int poismf_hip_session_topn_adjusted(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* adj_indptr,
                                     const sparse_ix* adj_indices, const real_t* adj_factor, int exclude_seen, const sparse_ix* excl_indptr,
                                     const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_adjusted_check(users, n_users, n_top, s->dimA, s->dimB, s->k, adj_indptr, adj_indices, adj_factor, excl_indptr,
                                                      excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_adjusted_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, adj_indptr, adj_indices, adj_factor,
                                        exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Diversified batched top-N from the resident (compact) factors (topn_diverse.hip; include/poismf_hip.h section 1p), ordered as the
// calls above and in the same scratch, which it may grow: the deep pool, then greedy MMR picks on the device.
int poismf_hip_session_topn_diverse(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, size_t pool, double lambda,
                                    const real_t* item_inv_norm, int exclude_seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                    sparse_ix* out_ix, real_t* out_score, real_t* out_value)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_diverse_check(users, n_users, n_top, pool, lambda, s->dimA, s->dimB, s->k, item_inv_norm, excl_indptr,
                                                     excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_diverse_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, pool, lambda, item_inv_norm,
                                       exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score,
                                       out_value);
}

// List-wise evaluation against the resident B (list_eval.hip; include/poismf_hip.h section 1q), ordered as the calls above and in the
// same scratch: the lists are the input, so neither A nor the CSR shard is read.
int poismf_hip_session_list_eval(poismf_hip_session* s, const sparse_ix* lists, size_t n_users, size_t n_list, const real_t* item_inv_norm,
                                 const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes, unsigned int* out_pos,
                                 long long* out_cos, unsigned int* out_len, unsigned int* exposure)
{
    if (n_users == 0) return 0;
    if (s == nullptr) return 2;
    if (const int rc = poismf_hip_list_eval_check(lists, n_users, n_list, s->dimB, s->k, item_inv_norm, test_indptr, test_indices, budget_bytes,
                                                  out_pos, out_cos, out_len, exposure))
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_list_eval_run(s->stream, s->dB, s->dimB, s->k, lists, n_users, n_list, item_inv_norm, test_indptr, test_indices,
                                    budget_bytes, &s->d_topn, &s->topn_cap, out_pos, out_cos, out_len, exposure);
}

// Batched top-N over per-user include lists from the resident (compact) factors (topn_include.hip; include/poismf_hip.h section 1h),
// ordered as the call above and in the same scratch.
int poismf_hip_session_topn_include(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* incl_indptr,
                                    const sparse_ix* incl_indices, int exclude_seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                    sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_include_check(users, n_users, n_top, s->dimA, s->dimB, s->k, incl_indptr, incl_indices, excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_include_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, incl_indptr, incl_indices,
                                       exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix, out_score);
}

// Batched top-N over candidate lists shared between users from the resident (compact) factors (topn_shared.hip; include/poismf_hip.h
// section 1i), ordered as the calls above and in the same scratch.
int poismf_hip_session_topn_shared(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* list_indptr,
                                   const sparse_ix* list_indices, size_t n_lists, const sparse_ix* list_of, int exclude_seen,
                                   const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_shared_check(users, n_users, n_top, s->dimA, s->dimB, s->k, list_indptr, list_indices, n_lists, list_of,
                                                    excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_topn_shared_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, n_top, list_indptr, list_indices, n_lists,
                                      list_of, exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_ix,
                                      out_score);
}

// Batched exact ranks from the resident (compact) factors (rank_batch.hip; include/poismf_hip.h section 1g), ordered as the call above.
// The scratch is the batched top-N's: either call grows it to what it needs and neither keeps anything in it between calls.
int poismf_hip_session_rank_batch(poismf_hip_session* s, const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr,
                                  const sparse_ix* test_indices, int exclude_seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                                  unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_batch_check(users, n_users, s->dimA, s->dimB, s->k, test_indptr, test_indices, excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_rank_batch_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, test_indptr, test_indices,
                                     exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_rank, out_n_adm);
}

// Batched exact ranks among per-user include lists from the resident (compact) factors (rank_include.hip; include/poismf_hip.h
// section 1j), ordered as the calls above and in the same scratch.
int poismf_hip_session_rank_include(poismf_hip_session* s, const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr,
                                    const sparse_ix* test_indices, const sparse_ix* incl_indptr, const sparse_ix* incl_indices, int exclude_seen,
                                    const sparse_ix* excl_indptr, const sparse_ix* excl_indices, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_include_check(users, n_users, s->dimA, s->dimB, s->k, test_indptr, test_indices, incl_indptr, incl_indices,
                                                     excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_rank_include_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, test_indptr, test_indices, incl_indptr,
                                       incl_indices, exclude_seen ? &seen : nullptr, excl_indptr, excl_indices, &s->d_topn, &s->topn_cap, out_rank,
                                       out_n_adm);
}

// Batched exact ranks among candidate lists shared between users from the resident (compact) factors (rank_shared.hip;
// include/poismf_hip.h section 1k), ordered as the calls above and in the same scratch.
int poismf_hip_session_rank_shared(poismf_hip_session* s, const sparse_ix* users, size_t n_users, const sparse_ix* test_indptr,
                                   const sparse_ix* test_indices, const sparse_ix* list_indptr, const sparse_ix* list_indices, size_t n_lists,
                                   const sparse_ix* list_of, int unite_test, int exclude_seen, const sparse_ix* excl_indptr,
                                   const sparse_ix* excl_indices, unsigned int* out_rank, unsigned int* out_n_adm)
{
    if (n_users == 0) return 0;
    if (s == nullptr || out_rank == nullptr || out_n_adm == nullptr) return 2;
    if (const int rc = poismf_hip_rank_shared_check(users, n_users, s->dimA, s->dimB, s->k, test_indptr, test_indices, list_indptr, list_indices,
                                                    n_lists, list_of, excl_indptr, excl_indices))
        return rc;
    PmfTopnSeen seen;
    if (exclude_seen && !session_seen(s, users, n_users, seen)) return 2;
    HIP_TRY(hipSetDevice(s->device));
    return poismf_hip_rank_shared_run(s->stream, s->dA, s->dB, s->dimB, s->k, false, users, n_users, test_indptr, test_indices, list_indptr,
                                      list_indices, n_lists, list_of, unite_test != 0, exclude_seen ? &seen : nullptr, excl_indptr, excl_indices,
                                      &s->d_topn, &s->topn_cap, out_rank, out_n_adm);
}

#ifdef PMF_PROBE
// development only: the head words of the team buffer (a -DPMF_PROBE build sums phase cycles of the last team launch in [8, 16))
extern "C" __attribute__((visibility("default"))) int poismf_hip_debug_team_head(poismf_hip_session* s, unsigned long long* out)
{
    if (s->d_team == nullptr) return 1;
    return pmf_download(out, s->d_team, 8 * TEAM_HEAD_WORDS, s->stream) != hipSuccess;
}
// development only (not in the header): the raw per-row counters of half `which`, which a -DPMF_PROBE build fills with stamps
extern "C" __attribute__((visibility("default"))) int poismf_hip_debug_eval_rows(poismf_hip_session* s, int which, unsigned* out, size_t n)
{
    Half& h = s->half[which ? 1 : 0];
    if (h.d_eval_rows == nullptr) return 1;
    return pmf_download(out, h.d_eval_rows, sizeof(unsigned) * std::min(n, h.row_end - h.row_begin), s->stream) != hipSuccess;
}
#endif

int poismf_hip_session_set_segments(poismf_hip_session* s, int which, int nseg)
{
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    Half& h = s->half[which ? 1 : 0];
    if (h.d_indptr == nullptr || finish_half(h, s->stream, nseg)) return -1;
    return (int)h.segs.size();
}

int poismf_hip_session_segment_rows(poismf_hip_session* s, int which, int seg, size_t* row_begin, size_t* row_end)
{
    const Half& h = s->half[which ? 1 : 0];
    if (seg < 0 || seg >= (int)h.segs.size()) return 1;
    *row_begin = h.row_begin + h.segs[seg].row_lo;
    *row_end = h.row_begin + h.segs[seg].row_hi;
    return 0;
}

}  // extern "C"
