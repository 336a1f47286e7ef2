// sn_draw.hpp -- the draw of section 1t (include/poismf_hip.h) as one wave carries it out, shared by the negative sampler
// (sample_negatives.hip) and the fused sampled ranks (rank_sampled.hip, section 1u), in the way philox.hpp is shared: both kernels call
// sn_draw_row, so a row is the same set in both.  The header's sequential rule "walk the draws upward, accept what is admissible and
// not accepted before, stop at m accepts or at the cap" is carried out 64 draws at a time; lane l of a round takes draw d0 + l:
//   draw      the ten Philox rounds, r = (w1 << 32) | w0, then j = (r dimB) >> 64, or t = (r W) >> 64 and the first item whose
//             inclusive prefix sum C_j exceeds t: a search in the coarse index (every stride-th entry of C, staged in LDS by the
//             caller), then at most ceil(log2(stride)) steps in C itself, which stays in L2.
//   admitted  the caller's test of (item): the sampler's is tb_excluded, the fused ranks' adds the user's held-out row.
//   accepted  an open-addressing table in LDS, one word per slot: (item << 8) | tag, items being below 2^24.  Tag 0 marks an item
//             accepted in an earlier round, tag l + 1 one claimed in this round by lane l.  A lane walks from its item's hash: an empty
//             slot is taken by atomicCAS; a slot that holds its item takes an atomicMin of the lane's word, which, the items being
//             equal, leaves the LOWEST lane -- the earliest draw -- in the slot.  A lane that reads its own word back is the item's
//             first occurrence; an earlier round's word (tag 0) is below every lane's and stays.  The winners then clear their tags.
//             The tag in the key's word takes the place of a companion owner word per slot and halves the table.
//   the cut   __ballot of the winners, a prefix popcount for each one's place, and the lanes with count + place < m append to the
//             row's list in LDS, unsorted; the m-th accept's draw gives `draws`.  Lanes at or past the cap never draw.
// Between rounds the table holds the accepted items only, fewer than m in at least 2 m slots; inside the last round it may hold up to
// 63 items that the cut then leaves out.  No float anywhere.  sn_stage_weights is the host side of the weighted draw.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "philox.hpp"

namespace {

constexpr size_t SN_MAX_M = POISMF_HIP_NEG_MAX_M;
constexpr size_t SN_MAX_ITEMS = (size_t)1 << 24;          // an item and a tag share a word
constexpr size_t SN_SMALL_M = 256;                        // longest row of the instances with one user per wave of a workgroup
constexpr unsigned SN_SMALL_SLOTS = 512;
constexpr unsigned SN_COARSE = 1024;                      // entries of the coarse index of C
constexpr unsigned SN_EMPTY = 0xffffffffu;                // (no word (item << 8) | tag: tags end at 64)
static_assert(SN_SMALL_SLOTS >= 2 * SN_SMALL_M && SN_SMALL_M + 63 < SN_SMALL_SLOTS, "the table never fills");

// what a draw depends on besides the user: the same for every user of a call
struct SnDraw {
    unsigned m, cap, dimB;
    unsigned log_slots;                   // table slots per user, a power of two
    unsigned key0, key1;
    const unsigned long long* C;          // [dimB] inclusive prefix sums of the weights
    const unsigned long long* coarse;     // [n_coarse] C at the last item of every block of `stride` items
    unsigned n_coarse, stride;
    unsigned long long W;                 // C[dimB - 1]
};

inline unsigned sn_pow2_at_least(size_t n)
{
    unsigned l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

// m, the cap, the key and the table's size: slots for SN_SMALL_M in the small instances, at least 2 m above
inline SnDraw sn_draw_of(size_t m, size_t dimB, uint64_t seed)
{
    SnDraw d = {};
    d.m = (unsigned)m;
    d.cap = (unsigned)POISMF_HIP_NEG_DRAWS(m);
    d.dimB = (unsigned)dimB;
    d.log_slots = m <= SN_SMALL_M ? sn_pow2_at_least(SN_SMALL_SLOTS) : sn_pow2_at_least(2 * m);
    d.key0 = (unsigned)(seed & 0xffffffffu);
    d.key1 = (unsigned)(seed >> 32);
    return d;
}

// The weighted draw's host side: the prefix sums by sequential integer additions, and every stride-th of them, uploaded once per call
// to d_C [dimB] and d_coarse [SN_COARSE].
inline hipError_t sn_stage_weights(SnDraw& d, const uint32_t* item_weight, size_t dimB, void* d_C, void* d_coarse, hipStream_t stream)
{
    std::vector<unsigned long long> hC, hcoarse;
    try { hC.resize(dimB); } catch (const std::bad_alloc&) { return hipErrorOutOfMemory; }
    unsigned long long acc = 0;
    for (size_t j = 0; j < dimB; j++) hC[j] = acc += item_weight[j];
    d.W = acc;
    d.stride = (unsigned)pmf_ceil_div(dimB, SN_COARSE);
    d.n_coarse = (unsigned)pmf_ceil_div(dimB, d.stride);
    for (size_t b = 0; b < d.n_coarse; b++) hcoarse.push_back(hC[std::min(dimB, (b + 1) * d.stride) - 1]);
    hipError_t e = pmf_upload(d_C, hC.data(), dimB * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = pmf_upload(d_coarse, hcoarse.data(), hcoarse.size() * sizeof(unsigned long long), stream);
    d.C = (const unsigned long long*)d_C;
    d.coarse = (const unsigned long long*)d_coarse;
    return e;
}

// the first item whose prefix sum exceeds t < W
__device__ __forceinline__ unsigned sn_weighted_item(const SnDraw& a, const unsigned long long* coarse, unsigned long long t)
{
    unsigned lo = 0, hi = a.n_coarse - 1;   // (coarse[n_coarse - 1] = W > t)
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if (coarse[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    unsigned jl = lo * a.stride, jh = min(jl + a.stride, a.dimB) - 1;   // (C[jh] is coarse[lo] > t, and everything before jl is <= t)
    while (jl < jh) {
        const unsigned mid = (jl + jh) / 2;
        if (a.C[mid] > t) jh = mid;
        else jl = mid + 1;
    }
    return jl;
}

// One wave draws the row of stream `stream`: the accepted items go to lst[0 .. count) in the order of their draws, count is returned and
// `draws` is what the row consumed.  tab: 2^log_slots words of LDS, which this call fills with SN_EMPTY first; coarse: the coarse index
// in LDS (WEIGHTED); admitted(j): item j is not in the user's exclusion set.  Called by a whole wave with uniform arguments.
template <bool WEIGHTED, class Admitted>
__device__ __forceinline__ unsigned sn_draw_row(const SnDraw& a, const unsigned long long* coarse, unsigned* tab, unsigned* lst,
                                                unsigned long long stream, unsigned lane, Admitted admitted, unsigned& draws)
{
    const unsigned slots = 1u << a.log_slots;
    for (unsigned s = lane; s < slots; s += 64) tab[s] = SN_EMPTY;
    tb_wave_sync();
    const uint32_t key[2] = { a.key0, a.key1 };
    const unsigned m = a.m;
    unsigned count = 0;
    draws = a.cap;
    for (unsigned d0 = 0; d0 < a.cap && count < m; d0 += 64) {
        const unsigned d = d0 + lane;
        unsigned j = 0;
        bool cand = false;
        if (d < a.cap) {
            const uint32_t ctr[4] = { d, 0u, (uint32_t)stream, (uint32_t)(stream >> 32) };
            uint32_t w[4];
            pmf_philox4x32_10(ctr, key, w);
            const unsigned long long r = ((unsigned long long)w[1] << 32) | w[0];
            j = WEIGHTED ? sn_weighted_item(a, coarse, __umul64hi(r, a.W)) : (unsigned)__umul64hi(r, (unsigned long long)a.dimB);
            cand = admitted(j);
        }
        const unsigned mine = (j << 8) | (lane + 1);
        unsigned slot = (j * 0x9E3779B1u) >> (32 - a.log_slots);
        if (cand) {
            for (;;) {
                const unsigned prev = atomicCAS(&tab[slot], SN_EMPTY, mine);
                if (prev == SN_EMPTY) break;
                if ((prev >> 8) == j) { atomicMin(&tab[slot], mine); break; }
                slot = (slot + 1) & (slots - 1);
            }
        }
        tb_wave_sync();
        const bool win = cand && tab[slot] == mine;   // (a later lane with the same item, or an item of an earlier round, reads another word)
        const unsigned long long won = __ballot(win);
        const unsigned place = count + (unsigned)__popcll(won & (((unsigned long long)1 << lane) - 1));
        if (win) {
            tab[slot] = j << 8;
            if (place < m) lst[place] = j;
        }
        const unsigned long long last = __ballot(win && place == m - 1);   // (at most one lane: the m-th accept)
        if (last) draws = d0 + (unsigned)__builtin_ctzll(last) + 1;
        count = min(m, count + (unsigned)__popcll(won));
        tb_wave_sync();
    }
    return count;
}

}  // namespace
