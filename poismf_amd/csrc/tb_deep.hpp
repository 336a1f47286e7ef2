// tb_deep.hpp -- the deep batched top-N (topn_deep.hip; include/poismf_hip.h section 1l): what the session (session.hip) hands to its
// core, the chunk loop and scratch layout it shares with the diversified top-N (topn_diverse.hip, section 1p), which consumes a
// chunk's rows on the device, and the in-LDS sort its kernel prunes a candidate list with
#pragma once
#include <cstddef>
#include <algorithm>
#include <functional>

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

// The core's chunk loop with the chunk's results left on the device: for every chunk of users, in order, the merged rows of
// TdLayout(n_users, n_top, dimB, extra_per_user, extra_fixed) at `base` (the caller has allocated them) are filled and
// consume(u0, nu, d_ix, d_score) is called with the chunk's first user, its users and its rows [nu x n_top] (empty entries TB_NONE and
// -inf); everything is enqueued on `stream`, and consume returns 0 to go on.  `seen`, when given, has been through
// poismf_hip_topn_seen_sorted.  Returns 0, 1 or what consume returned.
typedef std::function<int(size_t u0, size_t nu, const unsigned* d_ix, const real_t* d_score)> TdConsume;
int poismf_hip_topn_deep_chunks(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, unsigned char* base, size_t extra_per_user, size_t extra_fixed,
                                const TdConsume& consume);

namespace {

constexpr size_t TD_N_TOP_MAX = POISMF_HIP_TOPN_DEEP_MAX_N_TOP;
constexpr size_t TD_BUDGET = (size_t)POISMF_HIP_TOPN_DEEP_BUDGET_MB << 20;
constexpr unsigned TD_SORT_MIN = 128;                     // fewest entries td_sort orders: one exchange per lane and step
constexpr size_t TD_STAGE_MIN = 256;                      // smallest staging area of a wave in LDS: it also queues a pass's 16 x 16 scores
constexpr size_t TD_TARGET_WGS = 512;                     // items are split over workgroups until a chunk has about this many, two per CU ...
constexpr size_t TD_IDX_MAX = TB_BUDGET / 2 / sizeof(unsigned);   // exclusion indices a chunk may carry: section 1f's

// entries of a (user, slice) list in scratch: a power of two (td_sort) with max(n_top / 2, 64) slots or more above n_top -- a step of
// the walk may add 64 -- so that at depth a prune is paid once per n_top / 2 - 64 appends at least
inline size_t td_cap(size_t n_top)
{
    size_t cap = TD_SORT_MIN;
    while (cap < n_top + std::max<size_t>(n_top / 2, 64)) cap *= 2;
    return cap;
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.  extra_per_user / extra_fixed: bytes a
// caller that keeps the results on the device (topn_diverse.hip) needs beside them, per user of a chunk and once; the chunk shrinks so
// that total + chunk_users x extra_per_user + extra_fixed stays inside the budget.
struct TdLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t cap;              // entries of one (user, slice) list
    size_t list_rows;        // (user, slice) lists
    size_t users, ex_indptr, ex_indices, list_score, list_ix, out_score, out_ix, total;
    TdLayout(size_t n_users, size_t n_top, size_t dimB, size_t extra_per_user = 0, size_t extra_fixed = 0)
    {
        const size_t E = sizeof(real_t) + sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TD_N_TOP_MAX);
        dimB = std::min<size_t>(std::max<size_t>(dimB, 1), 0x7fffffffull);
        cap = td_cap(n_top);
        // lists: users x slices <= TB_TU x TD_TARGET_WGS + users + TB_TU  (tb_slices: at most target / tiles + 1 slices), results: users
        const size_t rest = TD_BUDGET - TD_IDX_MAX * sizeof(unsigned) - 256;   // (256: alignment of the seven parts)
        const size_t fixed = 16 + (TB_TU * TD_TARGET_WGS + TB_TU) * cap * E + extra_fixed;
        const size_t per_user = 8 + (cap + n_top) * E + extra_per_user;
        size_t uc = std::min((rest - fixed) / per_user, TB_CHUNK_USERS_MAX);
        uc -= uc % TB_TU;
        uc = std::min(uc, n_users);
        chunk_users = uc;
        idx_cap = std::min(TD_IDX_MAX, uc * dimB);                             // (no overflow: 2^18 x 2^31)
        const size_t item_tiles = pmf_ceil_div(dimB, TB_TJ);
        list_rows = std::min(uc * std::min(item_tiles, TD_TARGET_WGS), TB_TU * TD_TARGET_WGS + TB_TU + uc);
        TbTake take;
        users = take(uc * sizeof(unsigned));
        ex_indptr = take((uc + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        list_score = take(list_rows * cap * sizeof(real_t));
        list_ix = take(list_rows * cap * sizeof(unsigned));
        out_score = take(uc * n_top * sizeof(real_t));
        out_ix = take(uc * n_top * sizeof(unsigned));
        total = take.o;
    }
};
static_assert((TB_TU * TD_TARGET_WGS + TB_TU) * 2048 * 12 + 16 + TD_IDX_MAX * 4 + 256 + TB_TU * (8 + 3072 * 12) <= TD_BUDGET,
              "the budget holds the lists of TD_TARGET_WGS workgroups and a tile of users at the deepest n_top in double");

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
