// drivers.hip -- the drop-in drivers on top of a session: run_poismf (ref: src/poismf.c:435-632) with its outer A/B alternation, step
// schedule, early-stop logic, SIGINT plumbing and return codes; poismf_hip_session_run; factors_multiple (ref: src/pred.c:66-199) and the
// testing aids built on it; the self-test of wave_ops.hpp's log.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <csignal>
#include <ctime>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <vector>

#include "session.hpp"

// ---- self-test of wave_ops.hpp's d_log against the device library's log --------------------------------------------
__global__ __launch_bounds__(256) void selftest_log_kernel(unsigned long long n, unsigned long long* worst_ulp, unsigned* mismatched_specials)
{
    unsigned long long worst = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
        // arguments: a dense sweep of [1/4, 4] (where cancellation is worst), then 2^-1074 .. 2^1023 through bit patterns
        double x;
        if (i < n / 2) x = 0.25 + 3.75 * (double)i / (double)(n / 2);
        else {
            const unsigned long long j = i - n / 2, m = n - n / 2;
            const unsigned long long bits = (unsigned long long)((double)j / (double)m * (double)0x7fefffffffffffffULL);
            x = __builtin_bit_cast(double, bits ? bits : 1ULL);
        }
        const double a = d_log(x), b = d_log_lib(x);
        const long long ia = __builtin_bit_cast(long long, a), ib = __builtin_bit_cast(long long, b);
        const unsigned long long d = (unsigned long long)(ia > ib ? ia - ib : ib - ia);   // same sign: distance in ulps
        if ((ia < 0) == (ib < 0)) worst = d > worst ? d : worst;
        else if (a != b) worst = ~0ULL >> 1;
    }
    atomicMax(worst_ulp, worst);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double sp[6] = { 0.0, -0.0, -1.0, __builtin_inf(), -__builtin_inf(), __builtin_nan("") };
        unsigned bad = 0;
        for (int q = 0; q < 6; q++) {
            const double a = d_log(sp[q]), b = d_log_lib(sp[q]);
            const bool same = (a != a && b != b) || a == b;
            bad += same ? 0u : 1u;
        }
        *mismatched_specials = bad;
    }
}

// -------------------------------------------------------------------------------------------------
// run_poismf: the drop-in                                   ref: src/poismf.c:435-632
// -------------------------------------------------------------------------------------------------
static volatile sig_atomic_t g_should_stop = 0;
static bool g_handle_locked = false;
static std::mutex g_handle_mutex;
// the device-visible twin of the interrupt flag (pinned host memory; see on_sigint below): one word, allocated on first use, never freed
static volatile unsigned* g_stop_word = nullptr;

// The interrupt reaches the row loops of CG / TNCG within a row (ref: src/poismf.c:301, :360: the reference's row loops test
// should_stop_procedure before every row and skip the rest).  Rounds 1-4 looked at the flag between half-sweeps only: up to one half (config
// C5: 260 ms) of latency.  The flag now has a twin in PINNED HOST MEMORY that the device reads directly (HalfArgs::stop, system-scope loads
// next to every row ticket): the handler's own store is all it takes -- no thread, no copy, no kernel that would have to find a free CU
// behind the very workgroups it is meant to stop (a first version overwrote the device-side queue heads by hipMemsetAsync / hipMemcpyAsync:
// 14 .. 290 ms, depending on what the chip was running).  PG has no poll (neither has the reference's pg_iteration, quirk Q8).
static void on_sigint(int)
{
    g_should_stop = 1;  // the reference also prints here; fprintf is not async-signal-safe, so run_poismf reports it
    volatile unsigned* w = g_stop_word;
    if (w != nullptr) *w = 1u;
}
// (g_handle_mutex held, or single-threaded) the device-visible twin of the flag; nullptr if it cannot be had (the flag is then polled
// between half-sweeps only, as before)
static const unsigned* stop_word_for_device()
{
    static bool tried = false;
    static const bool off = getenv("POISMF_HIP_NO_ROW_INTERRUPT") != nullptr;   // testing knob
    if (off) return nullptr;
    if (!tried) {
        tried = true;
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && p != nullptr) {
            *(volatile unsigned*)p = g_should_stop ? 1u : 0u;
            g_stop_word = (volatile unsigned*)p;
        } else (void)hipGetLastError();
    }
    return (const unsigned*)g_stop_word;
}

// what the other units see of the two (session.hpp)
bool interrupt_requested() { return g_should_stop != 0; }
const unsigned* device_stop_word() { return (const unsigned*)g_stop_word; }

// SIGINT plumbing of one call (ref: src/poismf.c:444-455, :618-630): the first call in the process to get here installs
// the handler and restores the previous one on the way out; nested / concurrent calls share the flag.
namespace {
struct SigintScope {
    typedef void (*sig_fn)(int);
    sig_fn old_handler = nullptr;
    bool has_lock = false;
    void enter()
    {
        std::lock_guard<std::mutex> lk(g_handle_mutex);
        if (!g_handle_locked) {
            g_handle_locked = true;
            has_lock = true;
            g_should_stop = 0;
            (void)stop_word_for_device();
            if (g_stop_word != nullptr) *g_stop_word = 0u;
            old_handler = signal(SIGINT, on_sigint);
        }
    }
    int leave(int ret_code, bool handle_interrupt)
    {
        std::lock_guard<std::mutex> lk(g_handle_mutex);
        const bool stopped = g_should_stop != 0;
        if (stopped) fprintf(stderr, "Error: procedure was interrupted\n");
        if (stopped && ret_code != 1) ret_code = 2;
        if (has_lock) {
            signal(SIGINT, old_handler);
            g_handle_locked = false;
            g_should_stop = 0;
            if (g_stop_word != nullptr) *g_stop_word = 0u;
        }
        if (stopped && !handle_interrupt) raise(SIGINT);
        return ret_code;
    }
};

// The outer alternation on a session whose factors are set (ref: src/poismf.c:506-608).  Returns 0, or 1 on a device error.
// after_first_b: called once, right after the FIRST B half has been launched (run_poismf uploads the A side's matrix then: that half needs
// the CSC and the factors only, and the copy engine is idle while it runs)
int run_alternation(poismf_hip_session* s, const poismf_hip_params& p, size_t numiter, const std::function<int()>* after_first_b = nullptr)
{
    const int method = p.method;
    const real_t l2_reg = p.l2_reg;
    real_t step_size = p.step_size;
    const bool tn_stop = (method == POISMF_TNCG) && p.early_stop;
    bool stopped_earlyA = false, stopped_earlyB = false;
    for (size_t it = 0; it < numiter; it++) {
        if (g_should_stop) break;
        // quirk Q6: the divisor uses the step before halving and is reused by the A half
        const real_t cnst_div = 1. / (1. + 2. * l2_reg * step_size);

        // ---- B half first (quirk Q5) ----
        if (!(method == POISMF_TNCG && stopped_earlyB)) {
            size_t unchanged = 0;
            if (poismf_hip_half_sweep(s, 0, &p, step_size, cnst_div, tn_stop ? &unchanged : nullptr)) return 1;
            if (tn_stop) stopped_earlyB = ((double)unchanged / (double)s->dimB) >= .95;  // ref: :401-403 (quirk Q7)
        }
        if (it == 0) pmf_tl("first B half launched");
        if (it == 0 && after_first_b != nullptr && (*after_first_b)()) return 1;
        if (method == POISMF_PG) step_size *= 0.5;  // ref: :532-533
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (it == 0) pmf_tl("first B half done");
        if (team_check(s)) return 1;   // (a word of eight bytes, and only after a half that had team launches)
        if (g_should_stop) break;

        // ---- A half ----
        if (!(method == POISMF_TNCG && stopped_earlyA)) {
            size_t unchanged = 0;
            if (poismf_hip_half_sweep(s, 1, &p, step_size, cnst_div, tn_stop ? &unchanged : nullptr)) return 1;
            if (tn_stop) stopped_earlyA = ((double)unchanged / (double)s->dimA) >= .95;
        }
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (it == 0) pmf_tl("first A half done");
        if (team_check(s)) return 1;
        if (stopped_earlyA && stopped_earlyB) break;
    }
    return team_check(s);
}

// the solver's parameters of a drop-in call, as the session's entry points take them
poismf_hip_params params_of(real_t l2_reg, real_t l1_reg, real_t w_mult, real_t step_size, int method, bool limit_step, size_t maxupd,
                            bool early_stop, bool reuse_prev)
{
    poismf_hip_params p;
    p.l2_reg = l2_reg; p.l1_reg = l1_reg; p.w_mult = w_mult; p.step_size = step_size;
    p.method = method; p.limit_step = limit_step; p.maxupd = maxupd;
    p.early_stop = early_stop; p.reuse_prev = reuse_prev;
    return p;
}

}  // namespace

// -------------------------------------------------------------------------------------------------
// factors_multiple: latent factors of new rows with B fixed          ref: src/pred.c:66-199
// -------------------------------------------------------------------------------------------------
// The solve, on a session whose A half holds the new rows, whose dA holds their start and whose dB holds B: factors_multiple below sets such
// a session up and throws it away, the entry points of fold_in.hip run it on the guest of a resident session.  The same launches either way.
int fold_in_solve(poismf_hip_session* s, const real_t* Bsum, real_t l2_reg, real_t w_mult, real_t step_size, size_t niter, size_t maxupd,
                  int method, bool limit_step, bool reuse_mean)
{
    const size_t ks = s->k;
    std::vector<real_t> bs(ks);
    int rc = 0;
    poismf_hip_params p = params_of(l2_reg, 0, w_mult, step_size, method, limit_step, maxupd, false, reuse_mean);
    const bool weighted = w_mult != (real_t)1.;
    if (method == POISMF_PG) {                                    // ref: :152-169
        const real_t step0 = step_size;
        for (size_t it = 0; it < niter && !rc; it++) {
            for (size_t c = 0; c < ks; c++) bs[c] = weighted ? Bsum[c] : Bsum[c] * (-step_size);
            const real_t cnst_div = 1. / (1. + 2. * l2_reg * step_size);
            // w != 1: Bsum_w was scaled by -step at set-up (ref: :121-122) and again by -step here (ref: :162)
            rc = half_sweep_impl(s, 1, &p, step_size, cnst_div, nullptr, bs.data(), -step0, weighted ? -step_size : (real_t)1);
            step_size *= 0.5;
        }
    } else {
        for (size_t c = 0; c < ks; c++) bs[c] = Bsum[c];
        if (method == POISMF_CG) p.maxupd = maxupd * niter;      // ref: :175-178
        rc = half_sweep_impl(s, 1, &p, step_size, (real_t)1, nullptr, bs.data(), -step_size);
    }
    return rc;
}

namespace {
int factors_multiple_impl(real_t* A, real_t* B, real_t* Bsum, real_t* Amean, real_t* Xr, sparse_ix* Xr_indptr,
                                 sparse_ix* Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult, real_t step_size,
                                 size_t niter, size_t maxupd, int method, bool limit_step, bool reuse_mean, unsigned* decisions)
{
    pmf_last_hip_error() = hipSuccess;   // (what this call reports on failure is this call's error, not an earlier call's)
    const size_t ks = (size_t)k;
    const size_t nnz = Xr_indptr[dimA];
    // rows start at the mean of the fitted A, except TNCG without reuse_mean (1e-3, set in the kernel); ref: :144-147
    if (reuse_mean || method != POISMF_TNCG)
        for (size_t r = 0; r < dimA; r++) memcpy(A + r * ks, Amean, ks * sizeof(real_t));
    if (nnz == 0) {  // every row is empty: all three drivers zero such rows (quirk Q7)
        memset(A, 0, dimA * ks * sizeof(real_t));
        return 0;
    }
    size_t dimB = 0;  // the reference never needs the number of items; the device copy of B needs the rows in use
    for (size_t i = 0; i < nnz; i++) dimB = std::max(dimB, (size_t)Xr_indices[i] + 1);

    const int device = pmf_env_device();
    poismf_hip_session* s = nullptr;
    int rc = 0;
    if (poismf_hip_session_create(&s, device, nullptr, Xr, Xr_indptr, Xr_indices, nullptr, nullptr, nullptr, dimA, dimB, ks, 0,
                                  dimA, 0, 0) ||
        hipMemcpy(s->dA, A, dimA * ks * sizeof(real_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->dB, B, dimB * ks * sizeof(real_t), hipMemcpyHostToDevice) != hipSuccess) {
        rc = 1;
    } else {
        if (decisions != nullptr) poismf_hip_session_profile(s, 1);
        rc = fold_in_solve(s, Bsum, l2_reg, w_mult, step_size, niter, maxupd, method, limit_step, reuse_mean);
        if (!rc && (hipStreamSynchronize(s->stream) != hipSuccess ||
                    hipMemcpy(A, s->dA, dimA * ks * sizeof(real_t), hipMemcpyDeviceToHost) != hipSuccess))
            rc = 1;
        if (!rc) rc = team_check(s);
        if (!rc && decisions != nullptr) rc = poismf_hip_session_decisions(s, 1, decisions, dimA);
    }
    poismf_hip_session_destroy(s);
    if (rc) pmf_report_failure();
    return rc ? 1 : 0;
}
}  // namespace

extern "C" {

// run_poismf's loop on a session that already holds X and the starting factors (PoisMF.fit keeps the CSR / CSC it
// built on the device and never takes them through host memory).  Same return codes as run_poismf.
int poismf_hip_session_run(poismf_hip_session* s, const poismf_hip_params* p, size_t numiter, int handle_interrupt)
{
    SigintScope sig;
    sig.enter();
    pmf_last_hip_error() = hipSuccess;
    int ret_code = 0;
    if (hipSetDevice(s->device) != hipSuccess || run_alternation(s, *p, numiter)) {
        pmf_report_failure();
        ret_code = 1;
    }
    return sig.leave(ret_code, handle_interrupt != 0);
}

int run_poismf(real_t* A, real_t* Xr, sparse_ix* Xr_indptr, sparse_ix* Xr_indices, real_t* B, real_t* Xc,
               sparse_ix* Xc_indptr, sparse_ix* Xc_indices, const size_t dimA, const size_t dimB, const size_t k,
               const real_t l2_reg, const real_t l1_reg, const real_t w_mult, real_t step_size, const int method,
               const bool limit_step, const size_t numiter, const size_t maxupd, const bool early_stop,
               const bool reuse_prev, const bool handle_interrupt, const int nthreads)
{
    (void)nthreads;
    SigintScope sig;
    sig.enter();
    pmf_last_hip_error() = hipSuccess;

    int ret_code = 0;
    poismf_hip_session* s = nullptr;
    int device = pmf_env_device();

    const poismf_hip_params p = params_of(l2_reg, l1_reg, w_mult, step_size, method, limit_step, maxupd, early_stop, reuse_prev);
    {   // several GPUs of this node (POISMF_HIP_DEVICES=0,1,..): same call, same results, rows sharded over the devices
        const std::vector<int> devs = devices_from_env();
        if (devs.size() > 1) {
            if (run_poismf_multi(devs, A, Xr, Xr_indptr, Xr_indices, B, Xc, Xc_indptr, Xc_indices, dimA, dimB, k, p, numiter)) {
                pmf_report_failure();
                ret_code = 1;
            }
            return sig.leave(ret_code, handle_interrupt);
        }
        if (devs.size() == 1) device = devs[0];
    }
    // POISMF_HIP_VERBOSE=1: wall time of the phases of this call on stderr (development aid, scripts/time_abi.py)
    static const bool verbose = getenv("POISMF_HIP_VERBOSE") != nullptr;
    double t[5] = { 0, 0, 0, 0, 0 };
    auto now = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6; };
    t[0] = now();
    // The session is put together in the order the first iteration needs things: the B side's matrix (CSC) and the factors first; the A
    // side's matrix (CSR: a third of the call's PCIe bytes) is uploaded -- pinned chunks, second stream -- and its rows are sorted while
    // the first B half runs (round 4).  poismf_hip_session_create does the same two build_half calls back to back.
    pmf_tl(nullptr);
    s = session_alloc(device, nullptr, dimA, dimB, k);
    pmf_tl("session allocated (factors, streams)");
    bool bad = s == nullptr;
    HalfPending pendB;   // (the B side's row sort runs on the device while the host threads stage the factors)
    bad = bad || build_half(s->half[0], s->stream, Xc, Xc_indptr, Xc_indices, dimB, dimA, 0, dimB, device, &pendB);
    t[1] = now();
    bad = bad || poismf_hip_session_set_factors(s, A, B);
    pmf_tl("factors handed to the DMA queue");
    if (!bad) bad = finish_half_collect(s->half[0], s->stream, pendB) != 0;
    else if (s != nullptr) { pmf_free(pendB.d_flag, s->stream); pmf_free(pendB.d_len, s->stream); }
    pmf_tl("B side: lengths back, bins cut");
    t[2] = now();
    double t_csr = 0;
    const std::function<int()> upload_csr = [&]() -> int {
        const double t0 = now();
        HIP_TRY(hipSetDevice(device));
        if (build_half(s->half[1], s->aux_stream, Xr, Xr_indptr, Xr_indices, dimA, dimB, 0, dimA, device)) return 1;
        HIP_TRY(hipStreamSynchronize(s->aux_stream));
        t_csr = now() - t0;
        return 0;
    };
    static const bool no_overlap = getenv("POISMF_HIP_NO_UPLOAD_OVERLAP") != nullptr;   // testing knob: the whole matrix before anything runs
    if (!bad && (no_overlap || numiter == 0)) bad = upload_csr() != 0;
    bad = bad || run_alternation(s, p, numiter, (no_overlap || numiter == 0) ? nullptr : &upload_csr);
    t[3] = now();
    pmf_tl("iterations done");
    bad = bad || poismf_hip_session_get_factors(s, A, B);
    pmf_tl("factors back");
    t[4] = now();
    if (bad) {
        pmf_report_failure();   // "Error: out of memory." (ref: :501) only when it was one
        ret_code = 1;
    }
    poismf_hip_session_destroy(s);
    pmf_tl("session destroyed");
    if (verbose)
        fprintf(stderr, "run_poismf: session + B side of X (upload, sort rows) %.2f ms, factors up %.2f ms, %zu iterations %.2f ms (of which the A "
                        "side of X, uploaded under the first B half: %.2f ms), factors down %.2f ms, teardown %.2f ms\n", t[1] - t[0], t[2] - t[1],
                numiter, t[3] - t[2], t_csr, t[4] - t[3], now() - t[4]);
    return sig.leave(ret_code, handle_interrupt);
}

int factors_multiple(real_t* A, real_t* B, real_t* Bsum, real_t* Amean, real_t* Xr, sparse_ix* Xr_indptr,
                     sparse_ix* Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult, real_t step_size,
                     size_t niter, size_t maxupd, int method, bool limit_step, bool reuse_mean, int nthreads)
{
    (void)nthreads;
    return factors_multiple_impl(A, B, Bsum, Amean, Xr, Xr_indptr, Xr_indices, k, dimA, l2_reg, w_mult, step_size, niter, maxupd, method,
                                 limit_step, reuse_mean, nullptr);
}
// Testing aid (G1): the device's own objective and gradient wrappers at a given point, row by row, through whatever engine a CG
// half-sweep would use for rows of that length (plan.hpp, K_EVAL).  which = 0: fun_single + grad_single (ref: src/poismf.c:194-240);
// 1: fun_and_grad (ref: :242-273).  G [dimA x k] gets the gradients, f [dimA] the function values; every row is evaluated at `point`.
int poismf_hip_debug_row_eval(real_t* G, double* f, real_t* B, real_t* Bsum, real_t* point, real_t* Xr, sparse_ix* Xr_indptr,
                              sparse_ix* Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult, int which)
{
    std::vector<unsigned> dec;
    try { dec.assign(2 * dimA, 0u); } catch (const std::bad_alloc&) { return 1; }
    const int rc = factors_multiple_impl(G, B, Bsum, point, Xr, Xr_indptr, Xr_indices, k, dimA, l2_reg, w_mult, (real_t)1e-7, 1, which ? 1 : 0,
                                         POISMF_EVAL, true, true, dec.data());
    if (rc) return rc;
    for (size_t r = 0; r < dimA; r++) {
        const unsigned long long b = ((unsigned long long)dec[2 * r + 1] << 32) | dec[2 * r];
        memcpy(&f[r], &b, sizeof(double));
    }
    return 0;
}
// Testing aid: factors_multiple that also hands back every row's solver decisions (2 words per row, see
// poismf_hip_session_decisions) -- how the golden single-row fixtures pin the device's iteration / evaluation counts.
int poismf_hip_factors_multiple_decisions(real_t* A, real_t* B, real_t* Bsum, real_t* Amean, real_t* Xr, sparse_ix* Xr_indptr,
                                          sparse_ix* Xr_indices, int k, size_t dimA, real_t l2_reg, real_t w_mult, real_t step_size,
                                          size_t niter, size_t maxupd, int method, bool limit_step, bool reuse_mean, unsigned* decisions)
{
    return factors_multiple_impl(A, B, Bsum, Amean, Xr, Xr_indptr, Xr_indices, k, dimA, l2_reg, w_mult, step_size, niter, maxupd, method,
                                 limit_step, reuse_mean, decisions);
}

// Largest distance in ulps between this library's double log (wave_ops.hpp) and the device library's over n sample
// arguments, and the number of special arguments (+-0, -1, +-inf, NaN) on which they disagree.
int poismf_hip_selftest_log(size_t n, unsigned long long* worst_ulp, unsigned* mismatched_specials)
{
    unsigned long long* d_w = nullptr;
    unsigned* d_m = nullptr;
    HIP_TRY(hipMalloc(&d_w, sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&d_m, sizeof(unsigned)));
    HIP_TRY(hipMemset(d_w, 0, sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d_m, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(selftest_log_kernel, dim3(256 * 8), dim3(256), 0, 0, (unsigned long long)n, d_w, d_m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(worst_ulp, d_w, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mismatched_specials, d_m, sizeof(unsigned), hipMemcpyDeviceToHost));
    (void)hipFree(d_w);
    (void)hipFree(d_m);
    return 0;
}

#ifdef PMF_TIMING
// development-only export (not in the header): read and reset the phase timers (they live in the row-kernel translation unit)
__attribute__((visibility("default"))) void poismf_hip_debug_timing(unsigned long long* out) { (void)pmf_read_timing(out); }
#endif


}  // extern "C"
