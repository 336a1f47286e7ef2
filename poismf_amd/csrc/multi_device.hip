// multi_device.hip -- the in-process multi-device driver behind run_poismf (drivers.hip): one session and one host thread per listed device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "session.hpp"

// -------------------------------------------------------------------------------------------------
// Several GPUs behind the same C-ABI: POISMF_HIP_DEVICES=0,1,..,7 makes run_poismf cut the rows of A and of B into
// one contiguous, nnz-balanced range per listed device (ref: the row loops it shards are src/poismf.c:159-162, :296-299,
// :352-358), keep one session per device -- its shard of the CSR / CSC, both factors replicated -- and alternate with one host
// thread per device.  After a half every device holds the rows it updated; they travel DIRECTLY to every peer, device to
// device (hipMemcpyPeerAsync on the owner's stream: over xGMI's full mesh all seven links of a GPU carry one shard each at the
// same time; no staging, no collective to wait for the slowest rank), and the next half starts when all of them have landed.
// The k-vector column sums: every device needs the same bits, so the sum is cut into fixed blocks whose partial sums depend on the
// block number alone; device d computes its 1 / D of the blocks over its replica, the [blocks x k] partials travel like the rows, and
// every device runs the fixed-order second stage (round 5; rounds 2-4 had every device recompute the whole sum) -- which is what
// replaces the north-star's all-reduce with sharding-independent bits; TNCG's early-stop counter is summed on the host.
// A device may be listed more than once (POISMF_HIP_DEVICES=0,0): the shards then share that GPU, which is how the one-GPU
// test exercises every line of this path (tests/test_gpu_multi.py); results equal the single-session run bit for bit, since a
// row's arithmetic depends on its length class alone and the column sums are computed in one fixed order.
// -------------------------------------------------------------------------------------------------
namespace {

struct Range { size_t lo, hi; };
// contiguous row ranges with (nearly) equal nonzero counts: cuts at the nnz quantiles of the row pointers
std::vector<Range> balanced_ranges(const sparse_ix* indptr, size_t n, size_t parts)
{
    std::vector<Range> out;
    const unsigned long long total = (unsigned long long)indptr[n];
    size_t prev = 0;
    for (size_t pidx = 1; pidx <= parts; pidx++) {
        size_t cut = n;
        if (pidx < parts) {
            const unsigned long long target = total * pidx / parts;
            cut = (size_t)(std::lower_bound(indptr, indptr + n + 1, (sparse_ix)target) - indptr);
            cut = std::min(std::max(cut, prev), n);
        }
        out.push_back({ prev, cut });
        prev = cut;
    }
    return out;
}

// Host threads meet here; the LAST one to arrive runs `last` (decisions every thread must share) before anybody leaves.
struct HostBarrier {
    std::mutex m;
    std::condition_variable cv;
    size_t n, waiting = 0, generation = 0;
    explicit HostBarrier(size_t n_) : n(n_) {}
    template <class Fn> void arrive(Fn&& last)
    {
        std::unique_lock<std::mutex> lk(m);
        const size_t gen = generation;
        if (++waiting == n) {
            last();
            waiting = 0;
            generation++;
            cv.notify_all();
        } else cv.wait(lk, [&] { return generation != gen; });
    }
    void arrive() { arrive([] {}); }
};

// Round 4.  One PERSISTENT host thread per device runs the whole alternation for its device (round 3 created and joined a thread
// per device twice per half and synchronised every stream with the host in between: at C4 on 8 GPUs a PG half is ~0.65 ms per
// device, the same order as those).  Devices are ordered against each other by EVENTS only:
//   * after a half, device d copies the rows it updated straight into every peer's replica (hipMemcpyPeerAsync, xGMI full mesh) on a
//     COPY stream of its own, segment by segment (the A half is cut into segments, poismf_hip_session_set_segments): segment j
//     travels while segment j + 1 computes; the event landed[d] is recorded behind the last copy;
//   * before its next half, device d makes its session stream wait for landed[q] of every peer q.  That one wait covers all three
//     hazards: the rows the next half gathers have arrived; a peer finished READING factor M (as the fixed factor of its previous
//     half) before anybody's copies of M's new rows reach it (those copies follow kernels that waited for that peer's landed event);
//     and d's own copies of two halves ago are done before d overwrites the same rows again (every peer waited for them before
//     the half whose landed event d has just waited for).
//     (TNCG with early stop may skip a half: two CONSECUTIVE halves then update the same factor, and a device may overwrite rows whose
//     previous copies are still travelling.  Harmless: copies on one copy stream are issued and land in order, every reader of those rows waits for
//     the LATER half's landed event, and the replica of a peer ends up holding the later rows -- nobody reads in between.)
// A stream can only wait for an event that has been RECORDED, so the threads hand over "recorded" through an atomic counter per
// device (a host-side spin for the record CALL of a peer, never for the device); two events per device alternate.
// Host threads meet at a barrier once per outer iteration (interrupt flag and failures: everybody takes the same decision) and,
// for TNCG with early stop, once per half (the unchanged-row counts are summed, ref: src/poismf.c:395-403).
struct MultiRun {
    size_t nd;
    const std::vector<int>& devices;
    std::vector<Range> rA, rB;
    std::vector<poismf_hip_session*> ss;
    std::vector<hipStream_t> copy_stream;
    std::vector<hipEvent_t> seg_done;                  // "this segment's kernels are done": session stream -> copy stream
    std::vector<hipEvent_t> landed;                    // [2 d + parity]: device d's rows of a half have reached every peer
    std::unique_ptr<std::atomic<unsigned>[]> recorded; // halves of device d whose `landed` event has been recorded
    std::vector<hipEvent_t> part_done;                 // "this device's share of the column sums' first stage is done": session stream -> copy stream
    std::vector<hipEvent_t> part_landed;               // [2 d + parity]: device d's partial sums of a half have reached every peer
    std::unique_ptr<std::atomic<unsigned>[]> part_recorded;
    std::vector<size_t> unchanged;
    std::vector<hipError_t> err;
    std::atomic<int> failed{0};
    bool stop = false;                                 // decided at the iteration barrier
    HostBarrier bar;
    MultiRun(const std::vector<int>& devs, size_t dimA, size_t dimB, const sparse_ix* pA, const sparse_ix* pB)
        : nd(devs.size()), devices(devs), rA(balanced_ranges(pA, dimA, devs.size())), rB(balanced_ranges(pB, dimB, devs.size())),
          ss(nd, nullptr), copy_stream(nd, nullptr), seg_done(nd, nullptr), landed(2 * nd, nullptr),
          recorded(new std::atomic<unsigned>[nd]), part_done(nd, nullptr), part_landed(2 * nd, nullptr),
          part_recorded(new std::atomic<unsigned>[nd]), unchanged(nd, 0), err(nd, hipSuccess), bar(nd)
    {
        for (size_t d = 0; d < nd; d++) { recorded[d].store(0); part_recorded[d].store(0); }
    }
    void fail(size_t d)
    {
        if (err[d] == hipSuccess) err[d] = pmf_last_hip_error();
        failed.store(1);
    }
    // every peer's rows of half number `h` (0-based) have been copied into THIS device's replica: ordered before whatever is
    // issued next on the session stream
    int wait_for_peers(size_t d, unsigned h)
    {
        for (size_t q = 0; q < nd; q++) {
            if (q == d) continue;
            while (recorded[q].load(std::memory_order_acquire) < h + 1) {
                if (failed.load()) return 1;
                std::this_thread::yield();
            }
            HIP_TRY(hipStreamWaitEvent(ss[d]->stream, landed[2 * q + (h & 1u)], 0));
        }
        return 0;
    }
};

}  // namespace

int run_poismf_multi(const std::vector<int>& devices, real_t* A, real_t* Xr, sparse_ix* Xr_indptr, sparse_ix* Xr_indices, real_t* B, real_t* Xc,
                     sparse_ix* Xc_indptr, sparse_ix* Xc_indices, size_t dimA, size_t dimB, size_t k, const poismf_hip_params& p, size_t numiter)
{
    MultiRun R(devices, dimA, dimB, Xr_indptr, Xc_indptr);
    const size_t nd = R.nd;
    const int method = p.method;
    const bool tn_stop = (method == POISMF_TNCG) && p.early_stop;
    int want_seg = 4;   // segments of the A half (the B shards are a tenth of the size: one)
    if (const char* e = getenv("POISMF_HIP_MULTI_SEGMENTS")) want_seg = std::max(1, atoi(e));

    auto setup = [&](size_t d) -> int {
        if (poismf_hip_session_create(&R.ss[d], devices[d], nullptr, Xr, Xr_indptr, Xr_indices, Xc, Xc_indptr, Xc_indices, dimA, dimB, k,
                                      R.rA[d].lo, R.rA[d].hi, R.rB[d].lo, R.rB[d].hi)) return 1;
        if (poismf_hip_session_set_factors(R.ss[d], A, B)) return 1;
        HIP_TRY(hipSetDevice(devices[d]));
        HIP_TRY(hipStreamCreateWithFlags(&R.copy_stream[d], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&R.seg_done[d], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&R.landed[2 * d], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&R.landed[2 * d + 1], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&R.part_done[d], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&R.part_landed[2 * d], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&R.part_landed[2 * d + 1], hipEventDisableTiming));
        if (want_seg > 1 && poismf_hip_session_set_segments(R.ss[d], 1, want_seg) < 0) return 1;
        for (size_t q = 0; q < nd; q++)   // peer access where the pair allows it (the copies work without, staged by the runtime)
            if (devices[q] != devices[d]) { int can = 0; if (hipDeviceCanAccessPeer(&can, devices[d], devices[q]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[q], 0); }
        (void)hipGetLastError();
        return 0;
    };
    // one half on device d: its segments, each followed by the copies of its rows to every peer on the copy stream
    auto half = [&](size_t d, int which, unsigned h, real_t step, real_t cnst_div) -> int {
        poismf_hip_session* s = R.ss[d];
        if (h > 0) {
            if (R.wait_for_peers(d, h - 1)) return 1;
            poismf_hip_session_factors_dirty(s, which ? 0 : 1);   // the fixed factor of this half received rows: its gather copy is re-derived
        }
        // The first stage of this half's column sums is shared (poismf_hip_session_colsum_partial): device d sums its share of the
        // blocks over its whole replica, pushes those partial sums to every peer (copy stream, behind an event of the session stream), and
        // runs the fixed-order second stage once every peer's share has landed -- the unsharded sum bit for bit, 1 / nd of the first stage
        // per device.  Ordering: a peer sends its partials of half h only after it has waited for everybody's rows of half h - 1, i.e.
        // after this device's previous second stage (which read the array) and everything behind it; two events per device alternate,
        // handed over through a counter as the rows' `landed` events are.  Factors below shard_min rows are summed on every device.
        static const size_t shard_min = getenv("POISMF_SHARD_COLSUM_MIN_ROWS") ? (size_t)atoll(getenv("POISMF_SHARD_COLSUM_MIN_ROWS")) : (size_t)262144;
        if (nd > 1 && (which ? dimB : dimA) >= shard_min) {
            const int nb = poismf_hip_session_colsum_blocks(s, which);
            const int b_lo = (int)((size_t)nb * d / nd), b_hi = (int)((size_t)nb * (d + 1) / nd);
            if (poismf_hip_session_colsum_partial(s, which, b_lo, b_hi)) return 1;
            HIP_TRY(hipSetDevice(devices[d]));
            HIP_TRY(hipEventRecord(R.part_done[d], s->stream));
            HIP_TRY(hipStreamWaitEvent(R.copy_stream[d], R.part_done[d], 0));
            const size_t pbytes = (size_t)(b_hi - b_lo) * k * sizeof(real_t);
            for (size_t q = 0; q < nd && pbytes > 0; q++) {
                if (q == d) continue;
                HIP_TRY(hipMemcpyPeerAsync(poismf_hip_session_partials(R.ss[q]) + (size_t)b_lo * k, devices[q],
                                           poismf_hip_session_partials(s) + (size_t)b_lo * k, devices[d], pbytes, R.copy_stream[d]));
            }
            HIP_TRY(hipEventRecord(R.part_landed[2 * d + (h & 1u)], R.copy_stream[d]));
            R.part_recorded[d].store(h + 1, std::memory_order_release);
            for (size_t q = 0; q < nd; q++) {
                if (q == d) continue;
                while (R.part_recorded[q].load(std::memory_order_acquire) < h + 1) {
                    if (R.failed.load()) return 1;
                    std::this_thread::yield();
                }
                HIP_TRY(hipStreamWaitEvent(s->stream, R.part_landed[2 * q + (h & 1u)], 0));
            }
            poismf_hip_session_partials_ready(s);
        }
        const int nseg = (int)s->half[which].segs.size();
        R.unchanged[d] = 0;
        for (int j = 0; j < nseg; j++) {
            if (poismf_hip_half_sweep_segment(s, which, &p, step, cnst_div, j, tn_stop && j == nseg - 1 ? &R.unchanged[d] : nullptr)) return 1;
            HIP_TRY(hipSetDevice(devices[d]));
            size_t lo = 0, hi = 0;
            if (poismf_hip_session_segment_rows(s, which, j, &lo, &hi)) return 1;
            const size_t bytes = (hi - lo) * k * sizeof(real_t);
            HIP_TRY(hipEventRecord(R.seg_done[d], s->stream));
            HIP_TRY(hipStreamWaitEvent(R.copy_stream[d], R.seg_done[d], 0));
            real_t* mine = (which ? s->dA : s->dB) + lo * k;
            for (size_t q = 0; q < nd && bytes > 0; q++) {
                if (q == d) continue;
                real_t* theirs = (which ? R.ss[q]->dA : R.ss[q]->dB) + lo * k;
                HIP_TRY(hipMemcpyPeerAsync(theirs, devices[q], mine, devices[d], bytes, R.copy_stream[d]));
            }
        }
        HIP_TRY(hipEventRecord(R.landed[2 * d + (h & 1u)], R.copy_stream[d]));
        R.recorded[d].store(h + 1, std::memory_order_release);
        return 0;
    };
    auto worker = [&](size_t d) {
        pmf_last_hip_error() = hipSuccess;
        if (setup(d)) R.fail(d);
        R.bar.arrive();
        real_t step_size = p.step_size;
        bool stoppedA = false, stoppedB = false;
        unsigned h = 0;
        for (size_t it = 0; it < numiter; it++) {
            R.bar.arrive([&] { R.stop = interrupt_requested() || R.failed.load() != 0; });
            if (R.stop) break;
            const real_t cnst_div = 1. / (1. + 2. * p.l2_reg * step_size);                       // quirk Q6
            for (int which = 0; which < 2; which++) {                                           // B half first (quirk Q5)
                bool& stopped = which ? stoppedA : stoppedB;
                if (!(method == POISMF_TNCG && stopped)) {
                    if (!R.failed.load() && half(d, which, h, step_size, cnst_div)) R.fail(d);
                    h++;
                    if (tn_stop) {                                                              // ref: src/poismf.c:395-403
                        size_t total = 0;
                        R.bar.arrive();
                        for (size_t u : R.unchanged) total += u;
                        R.bar.arrive();   // (everybody has read the counts before the next half resets them)
                        stopped = ((double)total / (double)(which ? dimA : dimB)) >= .95;
                    }
                }
                if (which == 0 && method == POISMF_PG) step_size *= 0.5;                        // ref: :532-533
            }
            if (stoppedA && stoppedB) break;
        }
        // the last half's rows of every peer, then this device is done
        if (!R.failed.load() && h > 0 && R.ss[d] != nullptr) {
            if (R.wait_for_peers(d, h - 1)) R.fail(d);
            else if (hipSetDevice(devices[d]) != hipSuccess || hipStreamSynchronize(R.ss[d]->stream) != hipSuccess ||
                     hipStreamSynchronize(R.copy_stream[d]) != hipSuccess) { pmf_last_hip_error() = hipGetLastError(); R.fail(d); }
            else if (team_check(R.ss[d])) R.fail(d);
        }
        R.bar.arrive();
    };
    {
        std::vector<std::thread> th;
        for (size_t d = 1; d < nd; d++) th.emplace_back(worker, d);
        worker(0);
        for (auto& t : th) t.join();
    }
    int rc = R.failed.load() ? 1 : 0;
    if (rc) {   // the failing worker's error is what the caller reports (the workers' thread-local slots are gone)
        pmf_last_hip_error() = hipSuccess;
        for (hipError_t e : R.err) if (e != hipSuccess) { pmf_last_hip_error() = e; break; }
    }
    if (!rc) rc = poismf_hip_session_get_factors(R.ss[0], A, B);   // every replica holds the same bits
    for (size_t d = 0; d < nd; d++) {
        (void)hipSetDevice(devices[d]);
        if (R.copy_stream[d]) { (void)hipStreamSynchronize(R.copy_stream[d]); (void)hipStreamDestroy(R.copy_stream[d]); }
        if (R.seg_done[d]) (void)hipEventDestroy(R.seg_done[d]);
        for (int e = 0; e < 2; e++) if (R.landed[2 * d + e]) (void)hipEventDestroy(R.landed[2 * d + e]);
        if (R.part_done[d]) (void)hipEventDestroy(R.part_done[d]);
        for (int e = 0; e < 2; e++) if (R.part_landed[2 * d + e]) (void)hipEventDestroy(R.part_landed[2 * d + e]);
        poismf_hip_session_destroy(R.ss[d]);
    }
    return rc ? 1 : 0;
}

// POISMF_HIP_DEVICES: comma-separated device ids; empty / one entry: the single-device path
std::vector<int> devices_from_env()
{
    std::vector<int> out;
    const char* e = getenv("POISMF_HIP_DEVICES");
    if (e == nullptr) return out;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return out;
    for (const char* q = e; *q;) {
        char* end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q) break;
        if (v >= 0 && v < n) out.push_back((int)v);
        q = (*end == ',') ? end + 1 : end;
        if (*end != ',' && *end != 0) break;
    }
    return out;
}
