// tb_quota.hpp -- the group-aware selection of the batched top-N with per-group quotas (topn_quota.hip; include/poismf_hip.h section
// 1n): the prune of one user's candidate list in LDS and the merge of a user's per-slice lists, both by counting under the total order of
// tb_tile.hpp.  An entry is counted twice: against the entries of ITS OWN GROUP that come before it (q(g) of them or more: the entry is
// dead, whatever else is in the list), and, when it lives, against the live entries that come before it (its place in the answer).
// The two maps are per item and interleaved: item_map[j] = (g(j), min(q(g(j)), n_top)), so a count needs one look-up and none by group.
#pragma once
#include <limits>

#include <hip/hip_runtime.h>

#include "../../include/poismf_hip.h"
#include "tb_tile.hpp"

namespace {

constexpr int TQ_STAGE = TB_PRUNE_Q * 64;                 // words of a wave's group stage in LDS: one per entry a prune can hold

// tb_prune with quotas: rank-counts list `u` (c entries, c <= cap <= TQ_STAGE), drops every entry that has as many entries of its own
// group before it as its quota or more, keeps the best min(live, n_top) of the rest in order and, when n_top live entries exist, sets the
// user's threshold to the last of them.  One pass counts, for every entry, all the entries before it and those of its group among them;
// only when some entry died does a second pass take the dead ones out of the first count again.  gs: the wave's stage, TQ_STAGE words.
// item_map[j] = (g(j), quota of g(j)).  Called by a whole wave with uniform arguments.
__device__ __forceinline__ void tb_prune_quota(real_t* ls, unsigned* li, unsigned* gs, unsigned c, unsigned n_top, const uint2* item_map,
                                               unsigned* cnt_u, real_t* thr_s_u, unsigned* thr_j_u)
{
    const unsigned lane = threadIdx.x & 63;
    real_t es[TB_PRUNE_Q];
    unsigned ej[TB_PRUNE_Q], eg[TB_PRUNE_Q], eq[TB_PRUNE_Q], rk[TB_PRUNE_Q], same[TB_PRUNE_Q];
#pragma unroll
    for (int q = 0; q < TB_PRUNE_Q; q++) {
        const unsigned e = lane + 64u * q;
        es[q] = e < c ? ls[e] : (real_t)0;
        ej[q] = e < c ? li[e] : TB_NONE;
        const uint2 gq = e < c ? item_map[ej[q]] : make_uint2(TB_NONE, 0u);   // (read by a few lanes per prune; the map stays in L2)
        eg[q] = gq.x;
        eq[q] = gq.y;
        rk[q] = same[q] = 0;
        if (e < c) gs[e] = eg[q];
    }
    tb_wave_sync();
    for (unsigned i = 0; i < c; i++) {
        const real_t si = ls[i];
        const unsigned ji = li[i], gi = gs[i];
#pragma unroll
        for (int q = 0; q < TB_PRUNE_Q; q++) {
            const bool b = tb_better(si, ji, es[q], ej[q]);
            rk[q] += b ? 1u : 0u;
            same[q] += (b && gi == eg[q]) ? 1u : 0u;
        }
    }
    bool live[TB_PRUNE_Q];
    unsigned n_dead = 0;   // (uniform over the wave)
#pragma unroll
    for (int q = 0; q < TB_PRUNE_Q; q++) {
        const unsigned e = lane + 64u * q;
        live[q] = e < c && same[q] < eq[q];
        n_dead += (unsigned)__popcll(__ballot(e < c && !live[q]));
    }
    tb_wave_sync();
    if (n_dead) {
        // an entry's place in the answer counts the LIVE entries before it: mark the dead ones in the stage and take them out again
#pragma unroll
        for (int q = 0; q < TB_PRUNE_Q; q++) {
            const unsigned e = lane + 64u * q;
            if (e < c && !live[q]) gs[e] = TB_NONE;       // (no group: group ids are below 2^31)
        }
        tb_wave_sync();
        for (unsigned i = 0; i < c; i++) {
            if (gs[i] != TB_NONE) continue;               // (uniform)
            const real_t si = ls[i];
            const unsigned ji = li[i];
#pragma unroll
            for (int q = 0; q < TB_PRUNE_Q; q++) rk[q] -= tb_better(si, ji, es[q], ej[q]) ? 1u : 0u;
        }
        tb_wave_sync();
    }
#pragma unroll
    for (int q = 0; q < TB_PRUNE_Q; q++) {
        if (live[q] && rk[q] < n_top) {
            ls[rk[q]] = es[q];
            li[rk[q]] = ej[q];
            if (rk[q] == n_top - 1) { *thr_s_u = es[q]; *thr_j_u = ej[q]; }
        }
    }
    const unsigned n_live = c - n_dead;
    if (lane == 0) *cnt_u = n_live < n_top ? n_live : n_top;
    tb_wave_sync();
}

// tb_select.hpp's prune with quotas: the wave's stage and the map travel with it, so the selection knows nothing about groups
struct TbPruneQuota {
    unsigned* gs;            // this wave's stage, TQ_STAGE words
    const uint2* item_map;
    __device__ __forceinline__ void operator()(real_t* ls, unsigned* li, unsigned c, unsigned n_top, unsigned* cnt_u, real_t* thr_s_u, unsigned* thr_j_u) const
    {
        tb_prune_quota(ls, li, gs, c, n_top, item_map, cnt_u, thr_s_u, thr_j_u);
    }
};

// One wave (a workgroup of 64): the answer from nslices sorted partial lists of n_top entries each (part_*: the first of them; a short
// list ends in empty entries), by the same two counts over their union, to out_*[0 .. n_top); the ranks no live entry reaches are marked
// empty.  ms / mj / mg / mq: TB_MERGE_MAX entries of LDS each; n_live: one word of LDS.  Within a sorted list the entries that come
// before a given one form a prefix, so both counts leave a list at its first entry that does not.
__device__ __forceinline__ void tb_merge_lists_quota(real_t* ms, unsigned* mj, unsigned* mg, unsigned* mq, unsigned* n_live, const real_t* part_score,
                                                     const unsigned* part_ix, unsigned nslices, unsigned n_top, const uint2* item_map,
                                                     real_t* out_score, unsigned* out_ix)
{
    const unsigned lane = threadIdx.x;
    const unsigned m = nslices * n_top;
    for (unsigned i = lane; i < m; i += 64) {
        const unsigned j = part_ix[i];
        ms[i] = part_score[i];
        mj[i] = j;
        mg[i] = j == TB_NONE ? TB_NONE : item_map[j].x;
    }
    if (lane == 0) *n_live = 0;
    __syncthreads();
    // count 1: the entries of my group that come before me; mq[e] = 1 for a live entry
    for (unsigned e = lane; e < m; e += 64) {
        const real_t s = ms[e];
        const unsigned j = mj[e], g = mg[e];
        unsigned alive = 0;
        if (j != TB_NONE) {
            const unsigned quota = item_map[j].y;
            unsigned same = 0;
            for (unsigned sl = 0; sl < nslices && same < quota; sl++)
                for (unsigned i = sl * n_top; i < (sl + 1) * n_top; i++) {
                    if (!tb_better(ms[i], mj[i], s, j)) break;   // (empty entries are better than nothing; the entry itself ends its own list's run)
                    same += mg[i] == g ? 1u : 0u;
                }
            alive = same < quota ? 1u : 0u;
        }
        mq[e] = alive;
        if (alive) atomicAdd(n_live, 1u);   // (LDS, integer)
    }
    __syncthreads();
    const unsigned filled = *n_live < n_top ? *n_live : n_top;
    for (unsigned i = filled + lane; i < n_top; i += 64) {
        out_score[i] = -std::numeric_limits<real_t>::infinity();
        out_ix[i] = TB_NONE;
    }
    // count 2: the live entries that come before me
    for (unsigned e = lane; e < m; e += 64) {
        if (!mq[e]) continue;
        const real_t s = ms[e];
        const unsigned j = mj[e];
        unsigned rk = 0;
        for (unsigned sl = 0; sl < nslices && rk < n_top; sl++)
            for (unsigned i = sl * n_top; i < (sl + 1) * n_top; i++) {
                if (!tb_better(ms[i], mj[i], s, j)) break;
                rk += mq[i];
            }
        if (rk < n_top) { out_score[rk] = s; out_ix[rk] = j; }
    }
}

}  // namespace
