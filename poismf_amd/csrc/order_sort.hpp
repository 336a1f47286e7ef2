// order_sort.hpp -- the device pieces of the batched re-rank (order_include.hip; include/poismf_hip.h section 1s): bitonic networks
// under the total order tb_better on keys (score, item) held in REGISTERS, and the merge-path search and in-LDS merge of two sorted
// runs.  An empty key is (-inf, TB_NONE): every real key, a score of -inf included, comes before it, and two empty keys are equal --
// the only equal keys there are, so no exchange ever has to choose between them.
//
// A network's exchange at distance d pairs entry e with entry e ^ d; both owners look at both keys and each keeps the one its place
// asks for, so nothing is written back and nothing is exchanged twice.  Where the partner lives decides what an exchange costs:
//   one wave      (os_wave_sort)  entry e = 64 q + lane is register q of lane `lane`: d < 64 is a lane exchange (__shfl_xor), d >= 64
//                 a compare between two registers of the same lane.  No LDS, no barrier.
//   one workgroup (os_wg_sort)    entry e = 256 r + t is register r of thread t of 256: d < 64 a lane exchange, d >= 256 two registers
//                 of one thread, and only d = 64 and d = 128 -- two steps per stage -- go through LDS: every thread stores its keys,
//                 a barrier, every thread loads its partners'.
// All loops have constant bounds and are unrolled, so that every register index is a constant; a stage above the (uniform) number
// of entries in use is skipped as a whole.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "tb_tile.hpp"

namespace {

constexpr int OS_WG = 256;                                // threads of the workgroup network and of the merge
constexpr unsigned OS_MERGE_BLOCK = 1024;                 // entries of output one workgroup of the merge produces

__device__ __forceinline__ real_t os_none_score() { return (real_t)-__builtin_huge_val(); }   // -inf

// this place keeps its own key (s, j) or takes the partner's (so, jo): the better of the two if want_better, else the worse
__device__ __forceinline__ void os_take(real_t& s, unsigned& j, real_t so, unsigned jo, bool want_better)
{
    const bool take = want_better ? tb_better(so, jo, s, j) : tb_better(s, j, so, jo);
    s = take ? so : s;
    j = take ? jo : j;
}

// registers lo < hi of one thread, `fwd`: the run they belong to ends best first
__device__ __forceinline__ void os_pair(real_t& s_lo, unsigned& j_lo, real_t& s_hi, unsigned& j_hi, bool fwd)
{
    const bool swap = fwd ? tb_better(s_hi, j_hi, s_lo, j_lo) : tb_better(s_lo, j_lo, s_hi, j_hi);
    const real_t ts = s_lo;
    const unsigned tj = j_lo;
    s_lo = swap ? s_hi : s_lo;
    j_lo = swap ? j_hi : j_lo;
    s_hi = swap ? ts : s_hi;
    j_hi = swap ? tj : j_hi;
}

// One wave orders the 64 nq entries e = 64 q + lane, q < nq (nq a power of two <= Q, uniform), best first.
template <int Q> __device__ __forceinline__ void os_wave_sort(real_t (&s)[Q], unsigned (&j)[Q], unsigned nq, unsigned lane)
{
#pragma unroll
    for (int k2 = 2; k2 <= 64 * Q; k2 <<= 1) {
        if (k2 <= 64 * (int)nq) {
#pragma unroll
            for (int d = k2 >> 1; d > 0; d >>= 1) {
                if (d >= 64) {
                    const int dq = d >> 6;
#pragma unroll
                    for (int q = 0; q < Q; q++)
                        if ((q & dq) == 0 && (q | dq) < Q) os_pair(s[q], j[q], s[q | dq], j[q | dq], ((64 * q) & k2) == 0);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        const real_t so = __shfl_xor(s[q], d);
                        const unsigned jo = (unsigned)__shfl_xor((int)j[q], d);
                        const bool low = (lane & (unsigned)d) == 0, fwd = ((64u * q + lane) & (unsigned)k2) == 0;
                        os_take(s[q], j[q], so, jo, low == fwd);
                    }
                }
            }
        }
    }
}

// A workgroup of OS_WG threads orders the OS_WG x E entries e = OS_WG r + t, best first.  ss / sj: OS_WG x E entries of LDS, free to be
// overwritten on entry (a barrier opens every round trip); called by every thread.
template <int E> __device__ __forceinline__ void os_wg_sort(real_t (&s)[E], unsigned (&j)[E], real_t* ss, unsigned* sj, unsigned t)
{
#pragma unroll
    for (int k2 = 2; k2 <= OS_WG * E; k2 <<= 1) {
#pragma unroll
        for (int d = k2 >> 1; d > 0; d >>= 1) {
            if (d >= OS_WG) {
                const int dr = d / OS_WG;
#pragma unroll
                for (int r = 0; r < E; r++)
                    if ((r & dr) == 0 && (r | dr) < E) os_pair(s[r], j[r], s[r | dr], j[r | dr], ((OS_WG * r) & k2) == 0);
            } else if (d >= 64) {
                __syncthreads();   // every thread has read what the round trip before left
#pragma unroll
                for (int r = 0; r < E; r++) { ss[OS_WG * r + t] = s[r]; sj[OS_WG * r + t] = j[r]; }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < E; r++) {
                    const unsigned e = OS_WG * r + t;
                    const bool low = (t & (unsigned)d) == 0, fwd = (e & (unsigned)k2) == 0;
                    os_take(s[r], j[r], ss[e ^ (unsigned)d], sj[e ^ (unsigned)d], low == fwd);
                }
            } else {
#pragma unroll
                for (int r = 0; r < E; r++) {
                    const real_t so = __shfl_xor(s[r], d);
                    const unsigned jo = (unsigned)__shfl_xor((int)j[r], d);
                    const bool low = (t & (unsigned)d) == 0, fwd = ((OS_WG * r + t) & (unsigned)k2) == 0;
                    os_take(s[r], j[r], so, jo, low == fwd);
                }
            }
        }
    }
}

// ---- merging two sorted runs a [la] and b [lb], a's entry first where two are equal (empty keys only) ----
// merge path: how many of the first o entries of the merged run come from a.  a[i] is among them exactly when fewer than o - i entries
// of b come before it, that is when b[o - 1 - i] does not.
__device__ __forceinline__ unsigned os_merge_path(const real_t* as, const unsigned* aj, unsigned la, const real_t* bs, const unsigned* bj, unsigned lb,
                                                  unsigned o)
{
    unsigned lo = o > lb ? o - lb : 0, hi = o < la ? o : la;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (tb_better(bs[o - 1 - mid], bj[o - 1 - mid], as[mid], aj[mid])) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// entries of the sorted run (rs, rj) [n] that come before key (s, j); with `ties`, those equal to it as well
__device__ __forceinline__ unsigned os_before(const real_t* rs, const unsigned* rj, unsigned n, real_t s, unsigned j, bool ties)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        const bool before = ties ? !tb_better(s, j, rs[mid], rj[mid]) : tb_better(rs[mid], rj[mid], s, j);
        if (before) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace
