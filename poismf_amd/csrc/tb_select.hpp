// tb_select.hpp -- the selection behind the score tile of tb_tile.hpp, shared by the batched top-N kernels that keep their candidate
// lists in LDS (topn_batch.hip: topn_tile_kernel; topn_quota.hip: topn_quota_tile_kernel; topn_shared.hip: topn_shared_kernel;
// topn_weighted.hip: topn_weighted_tile_kernel), how the host sizes it, and the plain merge of the slices' lists (topn_merge_kernel).  Per workgroup: 64 candidate lists of `cap` entries (scores, items), per user a threshold (the n_top-th best so
// far, score and item), a counter and the user's row of A.  A score dies in registers unless it beats its user's threshold under the
// total order; a survivor is looked up in E(u) (tb_excluded) and appended through the LDS counter; a list is pruned by its wave alone,
// by rank counting, whenever fewer than TB_ROOM slots are left (a pass over 16 item columns can add 16 candidates to one user).  Arrival
// order in a list varies from run to run; ranks under a strict total order do not, so the output is deterministic.  No float atomics.
//
// What the kernels differ in stays with them: which item a tile column stands for and whether it is in range, where a tile row's user
// sits in the chunk (the row of its exclusion list and of its result), and the prune -- a template parameter: TbPrunePlain here, the
// quota kernel's own in tb_quota.hpp.  topn_deep.hip keeps a selection of its own (lists in scratch, survivors queued, room made once
// per step).
#pragma once
#include <algorithm>
#include <limits>

#include <hip/hip_runtime.h>

#include "tb_tile.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int TB_ROOM = 16;                               // free slots a list must have before a pass over 16 item columns
constexpr size_t TB_LDS_LIMIT = 156 * 1024;
static_assert(TB_N_TOP_MAX + TB_ROOM + 32 <= (size_t)TB_PRUNE_Q * 64, "a prune keeps a whole list in TB_PRUNE_Q registers per lane");

// LDS of a workgroup: the two factor tiles, the selection (64 lists of `cap` entries; threshold score and item, counter and row of A per
// user) and `extra` bytes of the kernel's own behind it
constexpr size_t tb_select_bytes(size_t cap) { return (size_t)TB_TU * cap * (sizeof(real_t) + 4) + (size_t)TB_TU * (sizeof(real_t) + 12); }
constexpr size_t tb_lds_bytes(size_t cap, size_t extra) { return 2 * (size_t)TB_TU * TB_KS * sizeof(real_t) + tb_select_bytes(cap) + extra; }

// The capacity of a list: n_top, the room of a pass, and slack that spaces the prunes out where LDS has it
inline size_t tb_select_cap(size_t n_top, size_t extra)
{
    size_t cap = n_top + TB_ROOM + std::min<size_t>(n_top, 32);
    while (tb_lds_bytes(cap, extra) > TB_LDS_LIMIT && cap > n_top + TB_ROOM) cap -= 16;
    return cap;
}

// the prune of a list by rank counting alone (tb_tile.hpp)
struct TbPrunePlain {
    __device__ __forceinline__ void operator()(real_t* ls, unsigned* li, unsigned c, unsigned n_top, unsigned* cnt_u, real_t* thr_s_u, unsigned* thr_j_u) const
    {
        tb_prune(ls, li, c, n_top, cnt_u, thr_s_u, thr_j_u);
    }
};

// Lane l of wave w holds, per pass, the scores of users 16 w + 4 (l >> 4) + r, r = 0 .. 3, against the item of column l & 15
// (tb_compute's layout); the lists of users 16 w .. 16 w + 15 belong to wave w alone.
template <class T, class Prune> struct TbSelect {
    T* Ls;                 // [TB_TU][cap] candidate scores
    unsigned* Li;          // [TB_TU][cap] candidate items
    T* thr_s;              // [TB_TU] threshold: score ...
    unsigned* thr_j;       // ... and item
    unsigned* cnt;         // [TB_TU] entries in the list
    unsigned* uid;         // [TB_TU] row of A, TB_NONE for a tile row without a user
    unsigned cap, n_top;
    Prune prune;
    // the thresholds of this lane's four users stay in registers between prunes (only this wave's prunes move them)
    T thr_reg[4];
    bool u_valid[4];
    bool dirty;            // (uniform over the wave) candidates were appended since the lists' room was last checked

    static __device__ __forceinline__ unsigned urow0() { return 16 * (threadIdx.x >> 6) + 4 * ((threadIdx.x & 63) >> 4); }

    // Carves tb_select_bytes(cap) bytes at `lds`; row_of(row) is tile row `row`'s row of A, or TB_NONE.  Ends with a workgroup barrier.
    template <class RowOf> __device__ __forceinline__ void init(unsigned char* lds, unsigned cap_, unsigned n_top_, Prune prune_, RowOf row_of)
    {
        Ls = (T*)lds;
        Li = (unsigned*)(Ls + (size_t)TB_TU * cap_);
        thr_s = (T*)(Li + (size_t)TB_TU * cap_);
        thr_j = (unsigned*)(thr_s + TB_TU);
        cnt = thr_j + TB_TU;
        uid = cnt + TB_TU;
        cap = cap_;
        n_top = n_top_;
        prune = prune_;
        const unsigned tid = threadIdx.x;
        if (tid < TB_TU) {
            uid[tid] = row_of(tid);
            cnt[tid] = 0;
            thr_s[tid] = -std::numeric_limits<T>::infinity();   // the empty entry: every real (s, j), a score of -inf included, beats it
            thr_j[tid] = TB_NONE;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) { thr_reg[r] = thr_s[urow0() + r]; u_valid[r] = uid[urow0() + r] != TB_NONE; }
        dirty = true;
    }

    // tile row `row`'s row of A as tb_walk wants it
    __device__ __forceinline__ long long user_row(int row) const { const unsigned r = uid[row]; return r == TB_NONE ? -1ll : (long long)r; }

    // list uu (whole wave, uniform uu): the count never passes cap -- an append past the end is dropped, not stored
    __device__ __forceinline__ void prune_list(unsigned uu)
    {
        prune(Ls + (size_t)uu * cap, Li + (size_t)uu * cap, cnt[uu] < cap ? cnt[uu] : cap, n_top, cnt + uu, thr_s + uu, thr_j + uu);
    }

    // One pass of 16 item columns: s4[r] is the score of this lane's user r against item j (in_range: the column stands for an item at
    // all); pos_of(uu) is tile row uu's position in the chunk.
    template <class PosOf> __device__ __forceinline__ void pass(const T (&s4)[4], unsigned j, bool in_range, const TbExcl& excl, PosOf pos_of)
    {
        const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const unsigned col = lane & 15, quad = lane >> 4;
        // the members the pass reads, as locals: through `this` the compiler re-derives them around the LDS stores below and keeps more
        // scalars live across the item loop (measured on topn_tile_kernel: 1.3 % of its time)
        T* const Ls = this->Ls;
        unsigned* const Li = this->Li;
        unsigned* const cnt = this->cnt;
        unsigned* const thr_j = this->thr_j;
        unsigned* const uid = this->uid;
        const unsigned cap = this->cap;
        if (dirty) {
            const unsigned c_mine = cnt[16 * wave + col];
            unsigned long long full = __ballot(quad == 0 && c_mine + TB_ROOM > cap);
            if (full) {
                while (full) {
                    const unsigned uu = 16 * wave + (unsigned)__builtin_ctzll(full);
                    full &= full - 1;
                    prune_list(uu);
                }
#pragma unroll
                for (int r = 0; r < 4; r++) thr_reg[r] = thr_s[urow0() + r];
            }
            dirty = false;
        }
        bool appended = false;
        if (in_range) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned uu = urow0() + r;
                const T s = s4[r];
                if (u_valid[r] && s >= thr_reg[r] && (s > thr_reg[r] || j < thr_j[uu]) && !tb_excluded(excl, pos_of(uu), uid[uu], j)) {
                    const unsigned pos = atomicAdd(&cnt[uu], 1u);   // (LDS, integer)
                    if (pos < cap) {   // (always: a pass adds at most TB_ROOM to a list that had as many slots free)
                        Ls[(size_t)uu * cap + pos] = s;
                        Li[(size_t)uu * cap + pos] = j;
                    }
                    appended = true;
                }
            }
        }
        if (__ballot(appended)) {
            dirty = true;
            tb_wave_sync();
        }
    }

    // The slice's answer per user: the best min(count, n_top) in order, the rest marked empty (-inf, TB_NONE), to row
    // [pos_of(uu)][slice] of part_* [chunk position][nslices][n_top].
    template <class PosOf> __device__ __forceinline__ void finish(T* part_score, unsigned* part_ix, unsigned nslices, unsigned slice, PosOf pos_of)
    {
        const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (unsigned q = 0; q < 16; q++) {
            const unsigned uu = 16 * wave + q;
            if (uid[uu] == TB_NONE) continue;   // (uniform over the wave)
            prune_list(uu);
            const unsigned c = cnt[uu];
            const size_t o = ((size_t)pos_of(uu) * nslices + slice) * n_top;
            for (unsigned i = lane; i < n_top; i += 64) {
                part_score[o + i] = i < c ? Ls[(size_t)uu * cap + i] : -std::numeric_limits<T>::infinity();
                part_ix[o + i] = i < c ? Li[(size_t)uu * cap + i] : TB_NONE;
            }
        }
    }
};

// One wave per user: the best n_top of its nslices sorted partial lists, [user][nslices][n_top] (topn_batch.hip, topn_weighted.hip).
// PAD: a user may have fewer than n_top real entries in all, and the ranks none of them reaches are marked empty (-inf, TB_NONE);
// without it they are left as they were (section 1f's checks see to it that there are none).
template <bool PAD>
__global__ __launch_bounds__(64) void topn_merge_kernel(const real_t* part_score, const unsigned* part_ix, unsigned n_users, unsigned nslices,
                                                        unsigned n_top, real_t* out_score, unsigned* out_ix)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX];
    const unsigned u = blockIdx.x;
    const size_t o = (size_t)u * nslices * n_top;
    tb_merge_lists(ms, mj, part_score + o, part_ix + o, nslices, n_top, out_score + (size_t)u * n_top, out_ix + (size_t)u * n_top);
    if constexpr (PAD) tb_merge_pad(mj, nslices, n_top, out_score + (size_t)u * n_top, out_ix + (size_t)u * n_top);
}

}  // namespace
