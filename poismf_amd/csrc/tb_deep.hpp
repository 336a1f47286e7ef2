// tb_deep.hpp -- the deep batched top-N (topn_deep.hip; include/poismf_hip.h section 1l): what the session (session.hip) hands to its
// core, and the in-LDS sort its kernel prunes a candidate list with
#pragma once
#include <cstddef>
#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "tb_tile.hpp"
#include "tb_batch.hpp"

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_deep_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                               const sparse_ix* excl_indptr, const sparse_ix* excl_indices);
// The core on device-resident factors, as poismf_hip_topn_batch_run (tb_batch.hpp).  Returns 0 or 1.
int poismf_hip_topn_deep_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                             const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                             const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score);

namespace {

constexpr size_t TD_N_TOP_MAX = POISMF_HIP_TOPN_DEEP_MAX_N_TOP;
constexpr size_t TD_BUDGET = (size_t)POISMF_HIP_TOPN_DEEP_BUDGET_MB << 20;
constexpr unsigned TD_SORT_MIN = 128;                     // fewest entries td_sort orders: one exchange per lane and step
constexpr size_t TD_STAGE_MIN = 256;                      // smallest staging area of a wave in LDS: it also queues a pass's 16 x 16 scores

// entries of a (user, slice) list in scratch: a power of two (td_sort) with max(n_top / 2, 64) slots or more above n_top -- a step of
// the walk may add 64 -- so that at depth a prune is paid once per n_top / 2 - 64 appends at least
inline size_t td_cap(size_t n_top)
{
    size_t cap = TD_SORT_MIN;
    while (cap < n_top + std::max<size_t>(n_top / 2, 64)) cap *= 2;
    return cap;
}

// global stores of this wave's lanes become visible to loads of its other lanes (the appends before a prune, a prune's write-back before
// the next one reads it): tb_wave_sync orders LDS only
__device__ __forceinline__ void td_global_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// One wave puts p entries of LDS (p a power of two >= TD_SORT_MIN) in the total order, best first: a bitonic network,
// log2(p) (log2(p) + 1) / 2 steps of p / 128 exchanges per lane -- 66 steps of 16 at p = 2048.  Equal entries are the empty ones only.
// A lane reads the pairs of four of its exchanges before it writes any of them back (the pairs of a step are disjoint), so that four
// LDS round trips overlap: a list's wave is alone on its SIMD at the deepest n_top, and nothing else hides that latency.
__device__ __forceinline__ void td_sort(real_t* ss, unsigned* sj, unsigned p)
{
    constexpr int Q = 4;
    const unsigned lane = threadIdx.x & 63;
    for (unsigned k2 = 2; k2 <= p; k2 <<= 1)
        for (unsigned j = k2 >> 1; j > 0; j >>= 1) {
            for (unsigned t0 = lane; t0 < p / 2; t0 += 64 * Q) {
                unsigned i[Q], ji[Q], jl[Q];
                real_t si[Q], sl[Q];
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const unsigned t = t0 + 64 * q;
                    i[q] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    if (t < p / 2) { si[q] = ss[i[q]]; sl[q] = ss[i[q] | j]; ji[q] = sj[i[q]]; jl[q] = sj[i[q] | j]; }
                }
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const bool fwd = (i[q] & k2) == 0;   // this run ends best first
                    if (t0 + 64 * q < p / 2 && (fwd ? tb_better(sl[q], jl[q], si[q], ji[q]) : tb_better(si[q], ji[q], sl[q], jl[q]))) {
                        ss[i[q]] = sl[q]; sj[i[q]] = jl[q];
                        ss[i[q] | j] = si[q]; sj[i[q] | j] = ji[q];
                    }
                }
            }
            tb_wave_sync();
        }
}

}  // namespace
