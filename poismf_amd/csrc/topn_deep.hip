// topn_deep.hip -- deep batched top-N (include/poismf_hip.h, section 1l): section 1f's answer for n_top up to 1024, a short row padded.
//
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t   (tb_tile.hpp)
//
// The walk and the exclusion look-up are tb_tile.hpp's.  The selection is this file's own (tb_select.hpp's serves the kernels whose lists
// fit LDS), with the same threshold test.  A workgroup of four waves owns 64 users and a slice of
// the items, scores 64 x 64 at a time (fp32 on the f32 MFMA, fp64 on the VALU chain) and lets a score die in registers unless it beats
// the user's threshold (the n_top-th best so far; registers, with its copy and the item in LDS).  What differs is where a survivor goes,
// and that a pass's survivors are queued in LDS first, so that their exclusion look-ups run side by side over the lanes.
// At this depth 64 lists do not fit LDS, so a list lives in the call's scratch, [user][slice][cap] with cap = td_cap(n_top) a power of
// two; the append position still comes from an integer counter in LDS.  A list belongs to one wave.  Whenever fewer than 64 slots are
// free (a step over 64 item columns can add 64 candidates to one user) the wave stages the list into its own LDS area, orders it with a
// bitonic network (td_sort) and writes the best n_top back in order; the threshold becomes the last of them.  The appends are global
// stores of some lanes read back by others, so a workgroup-scope fence stands between them (td_global_sync).  Arrival order in a list
// varies from run to run; positions under a strict total order do not, so the output is deterministic.
// topn_deep_merge_kernel gives an entry of a user's nslices sorted lists its final position: its position in its own list plus, for every
// other list, the number of entries there that come before it (binary search).  Nothing of the merge lives in LDS but one counter.
// With one slice the tile kernel writes the results itself.  No float atomics anywhere.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_DEEP_BUDGET_MB holds a
// chunk's user list, exclusion lists, candidate lists and results (TdLayout, tb_deep.hpp; poismf_hip_topn_deep_scratch_bytes reports its
// size).  The chunk loop, poismf_hip_topn_deep_chunks, hands a chunk's merged rows to a callable while they are still on the device: the
// deep entry points fetch them, the diversified top-N (topn_diverse.hip) picks from them there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_deep.hpp"

namespace {

constexpr int TD_ROOM = TB_TJ;                            // free slots a list must have before a step over 64 item columns
constexpr size_t TD_LDS_LIMIT = 156 * 1024;
constexpr size_t TD_LDS_CU = 160 * 1024;                  // TD_TARGET_WGS (tb_deep.hpp) workgroups, two per CU, or one per CU where a CU's LDS holds
                                                          // only one: a second round of workgroups would add lists to fill, prune and merge,
                                                          // and no parallelism
constexpr int TD_MERGE_WG = 256;

struct TdArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in scratch
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users
    real_t* list_score;               // [n_users][nslices][cap]
    unsigned* list_ix;
    real_t* fin_score;                // where a slice's sorted best n_top go: [n_users][nslices][fin_stride]
    unsigned* fin_ix;
    unsigned fin_stride;
};

template <class T, bool MFMA> __global__ __launch_bounds__(TB_WG) void topn_deep_tile_kernel(TdArgs a)
{
    extern __shared__ __align__(16) unsigned char td_smem[];
    T* As = (T*)td_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    const size_t stage = a.cap > TD_STAGE_MIN ? a.cap : TD_STAGE_MIN;
    T* Ss = Bs + TB_TJ * TB_KS;                           // [4 waves][stage] staged scores of the list being pruned
    unsigned* Sj = (unsigned*)(Ss + 4 * stage);           // [4 waves][stage] ... and items
    T* thr_s = (T*)(Sj + 4 * stage);                      // [TB_TU] threshold: score ...
    unsigned* thr_j = (unsigned*)(thr_s + TB_TU);         // ... and item
    unsigned* cnt = thr_j + TB_TU;                        // [TB_TU] entries in the list
    unsigned* uid = cnt + TB_TU;                          // [TB_TU] row of A, TB_NONE beyond the chunk

    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned u_base = blockIdx.x * TB_TU;
    const T neg_inf = -std::numeric_limits<T>::infinity();
    if (tid < TB_TU) {
        const unsigned u = u_base + tid;
        uid[tid] = u < a.n_users ? a.users[u] : TB_NONE;
        cnt[tid] = 0;
        thr_s[tid] = neg_inf;                             // the empty entry: every real (s, j), a score of -inf included, beats it
        thr_j[tid] = TB_NONE;
    }
    __syncthreads();

    const unsigned ntiles = (a.dimB + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned col = lane & 15, quad = lane >> 4;
    const unsigned urow0 = 16 * wave + 4 * quad;          // this lane's four users are urow0 .. urow0 + 3
    auto user_row = [&](int row) { const unsigned r = uid[row]; return r == TB_NONE ? -1ll : (long long)r; };
    auto list_of = [&](unsigned uu) { return ((size_t)(u_base + uu) * a.nslices + blockIdx.y) * a.cap; };

    // Orders list uu (whole wave, uniform arguments).  In the walk: the best min(count, n_top) go back to the list in order, the count and,
    // once the list is full, the threshold follow.  At the end (`last`): they go to fin_*, the rest of the row marked empty.
    T* ss = Ss + (size_t)wave * stage;
    unsigned* sj = Sj + (size_t)wave * stage;
    auto prune = [&](unsigned uu, bool last) {
        T* gs = a.list_score + list_of(uu);
        unsigned* gj = a.list_ix + list_of(uu);
        const unsigned c = cnt[uu] < a.cap ? cnt[uu] : a.cap;
        unsigned p = TD_SORT_MIN;
        while (p < c) p <<= 1;                            // (p <= cap: cap is a power of two >= TD_SORT_MIN)
        td_global_sync();
        for (unsigned i = lane; i < p; i += 64) {
            ss[i] = i < c ? gs[i] : neg_inf;
            sj[i] = i < c ? gj[i] : TB_NONE;
        }
        tb_wave_sync();
        td_sort(ss, sj, p);
        const unsigned keep = c < a.n_top ? c : a.n_top;
        if (!last) {
            for (unsigned i = lane; i < keep; i += 64) { gs[i] = ss[i]; gj[i] = sj[i]; }
            if (lane == 0) {
                cnt[uu] = keep;
                if (c >= a.n_top) { thr_s[uu] = ss[a.n_top - 1]; thr_j[uu] = sj[a.n_top - 1]; }
            }
        } else {
            const size_t o = ((size_t)(u_base + uu) * a.nslices + blockIdx.y) * a.fin_stride;
            for (unsigned i = lane; i < a.n_top; i += 64) {
                a.fin_score[o + i] = i < keep ? ss[i] : neg_inf;
                a.fin_ix[o + i] = i < keep ? sj[i] : TB_NONE;
            }
        }
        tb_wave_sync();
        td_global_sync();
    };

    // the thresholds of this lane's four users stay in registers between prunes (only this wave's prunes move them)
    T thr_reg[4];
    bool u_valid[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { thr_reg[r] = thr_s[urow0 + r]; u_valid[r] = uid[urow0 + r] != TB_NONE; }
    bool dirty = true;   // (uniform over the wave) candidates were appended since the lists' room was last checked

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, tb_all_items(a.dimB), [&](T (&acc)[4][4], unsigned j_base) {
        // ---- selection: four passes of 16 item columns; the lists of users 16 wave .. 16 wave + 15 belong to this wave alone.  Room is
        // made once per step, for all four passes (TD_ROOM), so the sort's code stands in the loop once ----
        if (dirty) {
            const unsigned c_mine = cnt[16 * wave + col];
            unsigned long long full = __ballot(quad == 0 && c_mine + TD_ROOM > a.cap);
            if (full) {
                while (full) {
                    const unsigned uu = 16 * wave + (unsigned)__builtin_ctzll(full);
                    full &= full - 1;
                    prune(uu, false);
                }
#pragma unroll
                for (int r = 0; r < 4; r++) thr_reg[r] = thr_s[urow0 + r];
            }
            dirty = false;
        }
        // A pass: the scores that beat their user's threshold are queued in the wave's staging area (free between prunes; ballots give
        // the positions), then the queue is looked up in the exclusion lists and appended 64 entries at a time.  Deep lists keep a good
        // part of a tile alive, and a look-up is a chain of dependent loads: one per queue entry, side by side over the lanes, costs a
        // pass as many round trips as it has survivors / 64, not one per (user, item) slot of a lane.
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            unsigned nq = 0;   // (uniform over the wave)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned uu = urow0 + r;
                const T s = acc[t][r];
                const bool alive = j < a.dimB && u_valid[r] && s >= thr_reg[r] && (s > thr_reg[r] || j < thr_j[uu]);
                const unsigned long long m = __ballot(alive);
                if (alive) {
                    const unsigned q = nq + (unsigned)__popcll(m & ((1ull << lane) - 1));
                    ss[q] = s;
                    sj[q] = (uu << 6) | (16 * t + col);   // the wave's user row and the item's place in the tile
                }
                nq += (unsigned)__popcll(m);
            }
            if (nq) {
                tb_wave_sync();
                for (unsigned e = lane; e < nq; e += 64) {   // (nq <= 256 = TD_STAGE_MIN)
                    const T s = ss[e];
                    const unsigned uu = sj[e] >> 6, jj = j_base + (sj[e] & 63);
                    if (!tb_excluded(a.excl, u_base + uu, uid[uu], jj)) {
                        const unsigned pos = atomicAdd(&cnt[uu], 1u);   // (LDS, integer)
                        if (pos < a.cap) {   // (always: a step adds at most TD_ROOM to a list that had as many slots free)
                            a.list_score[list_of(uu) + pos] = s;
                            a.list_ix[list_of(uu) + pos] = jj;
                        }
                    }
                }
                dirty = true;
                tb_wave_sync();
            }
        }
    });

    // ---- the slice's answer per user: the best min(count, n_top) in order, the rest marked empty ----
    for (unsigned q = 0; q < 16; q++) {
        const unsigned uu = 16 * wave + q;
        if (uid[uu] == TB_NONE) continue;   // (uniform over the wave)
        prune(uu, true);
    }
}

// One workgroup per user: the best n_top of its nslices sorted lists of n_top entries, list sl at lists + sl cap.  An entry's final
// position is its position in its own list plus the number of entries of every other list that come before it; empty entries
// (-inf, TB_NONE) end every list and come before nothing.  Positions the real entries do not reach are marked empty.
__global__ __launch_bounds__(TD_MERGE_WG) void topn_deep_merge_kernel(const real_t* list_score, const unsigned* list_ix, unsigned nslices,
                                                                      unsigned cap, unsigned n_top, real_t* out_score, unsigned* out_ix)
{
    __shared__ unsigned n_real;
    const unsigned tid = threadIdx.x;
    const size_t o = (size_t)blockIdx.x * nslices * cap;
    const real_t* ls = list_score + o;
    const unsigned* lj = list_ix + o;
    real_t* os = out_score + (size_t)blockIdx.x * n_top;
    unsigned* oj = out_ix + (size_t)blockIdx.x * n_top;
    if (tid == 0) n_real = 0;
    __syncthreads();
    for (unsigned sl = tid; sl < nslices; sl += TD_MERGE_WG) {
        unsigned lo = 0, hi = n_top;   // the list's real entries: the first lo
        while (lo < hi) {
            const unsigned mid = (lo + hi) / 2;
            if (lj[(size_t)sl * cap + mid] != TB_NONE) lo = mid + 1;
            else hi = mid;
        }
        atomicAdd(&n_real, lo);        // (LDS, integer; nslices n_top < 2^32)
    }
    __syncthreads();
    for (unsigned i = (n_real < n_top ? n_real : n_top) + tid; i < n_top; i += TD_MERGE_WG) {
        os[i] = -std::numeric_limits<real_t>::infinity();
        oj[i] = TB_NONE;
    }
    const unsigned m = nslices * n_top;
    for (unsigned e = tid; e < m; e += TD_MERGE_WG) {
        const unsigned own = e / n_top;
        unsigned rk = e % n_top;
        const real_t s = ls[(size_t)own * cap + rk];
        const unsigned j = lj[(size_t)own * cap + rk];
        if (j == TB_NONE) continue;
        for (unsigned sl = 0; sl < nslices && rk < n_top; sl++) {
            if (sl == own) continue;
            const real_t* ps = ls + (size_t)sl * cap;
            const unsigned* pj = lj + (size_t)sl * cap;
            unsigned lo = 0, hi = n_top - rk;   // (n_top - rk better entries or more put this one past the end either way)
            while (lo < hi) {
                const unsigned mid = (lo + hi) / 2;
                if (tb_better(ps[mid], pj[mid], s, j)) lo = mid + 1;
                else hi = mid;
            }
            rk += lo;
        }
        if (rk < n_top) { os[rk] = s; oj[rk] = j; }
    }
}

size_t td_lds_bytes(size_t cap)
{
    return 2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + 4 * std::max(cap, TD_STAGE_MIN) * (sizeof(real_t) + 4) + (size_t)TB_TU * (sizeof(real_t) + 12);
}
static_assert(2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + 4 * 2048 * (sizeof(real_t) + 4) + (size_t)TB_TU * (sizeof(real_t) + 12) <= TD_LDS_LIMIT,
              "the two tiles and four staging areas of the deepest list fit LDS");

}  // namespace

extern "C" size_t poismf_hip_topn_deep_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TdLayout(n_users, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_deep_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                               const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TD_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TD_IDX_MAX)) return 2;
    return 0;
}

// ---- the chunk loop (tb_deep.hpp): a chunk's merged rows stay on the device for `consume` ----
int poismf_hip_topn_deep_chunks(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, unsigned char* base, size_t extra_per_user, size_t extra_fixed,
                                const TdConsume& consume)
{
    const TdLayout L(n_users, n_top, dimB, extra_per_user, extra_fixed);
    const size_t lds = td_lds_bytes(L.cap);
    if (lds > TD_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the deepest list)
    auto kern = topn_deep_tile_kernel<real_t, sizeof(real_t) == 4>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TD_LDS_LIMIT));

    TdArgs a;
    std::vector<unsigned> hu, hp, hx;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose exclusion lists fit the index area together
        // (the check bounds a row by the area's smallest size: every row fits)
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, 2 * lds > TD_LDS_CU ? TD_TARGET_WGS / 2 : TD_TARGET_WGS);
        const size_t nslices = sl.nslices;
        if (nu * nslices > L.list_rows) return 1;   // (cannot happen: TdLayout sizes the lists for any slicing of a chunk)
        a.A = dA;
        a.B = dB;
        a.users = (const unsigned*)(base + L.users);
        a.n_users = (unsigned)nu;
        a.dimB = (unsigned)dimB;
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.cap = (unsigned)L.cap;
        a.nslices = (unsigned)nslices;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        a.list_score = (real_t*)(base + L.list_score);
        a.list_ix = (unsigned*)(base + L.list_ix);
        // (one slice: its sorted lists are the results; more: they stay at the head of the lists for the merge)
        a.fin_score = nslices == 1 ? (real_t*)(base + L.out_score) : a.list_score;
        a.fin_ix = nslices == 1 ? (unsigned*)(base + L.out_ix) : a.list_ix;
        a.fin_stride = (unsigned)(nslices == 1 ? n_top : L.cap);
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            hipLaunchKernelGGL(topn_deep_merge_kernel, dim3((unsigned)nu), dim3(TD_MERGE_WG), 0, stream, a.list_score, a.list_ix, (unsigned)nslices,
                               (unsigned)L.cap, (unsigned)n_top, (real_t*)(base + L.out_score), (unsigned*)(base + L.out_ix));
            TB_TRY(hipGetLastError());
        }
        if (const int rc = consume(u0, nu, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score))) return rc;
        u0 = u1;
    }
    return 0;
}

// ---- core on device-resident factors (tb_deep.hpp) ----
int poismf_hip_topn_deep_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                             const sparse_ix* users, size_t n_users, size_t n_top, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                             const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const TdLayout L(n_users, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    std::vector<unsigned> hix;
    return poismf_hip_topn_deep_chunks(stream, dA, dB, dimB, k, compact_A, users, n_users, n_top, seen, excl_indptr, excl_indices,
                                       (unsigned char*)*d_scratch, 0, 0, [&](size_t u0, size_t nu, const unsigned* d_ix, const real_t* d_score) {
                                           return tb_fetch_results(u0, nu, n_top, d_ix, d_score, hix, out_ix, out_score, stream);
                                       });
}

extern "C" {

int poismf_hip_topn_deep(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                         size_t n_top, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_deep_check(users, n_users, n_top, dimA, dimB, (size_t)k, excl_indptr, excl_indices)) return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_deep_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, nullptr, excl_indptr,
                                                         excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
