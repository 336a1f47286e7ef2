// session_holdout.hip -- the seeded leave-out split (include/poismf_hip.h section 2f): which cells of a CSR's rows are held out is decided on
// the device from a Philox key per cell, (seed, user, item) -> 64 bits, and nothing else; the held-out cells of a resident session come
// back as a CSR and leave the resident matrix through section 2c's removal while their triplets are still on the device.
//
// Per listed row: h = min(n_out, #{cells with w0 < thresh}, max(len - min_keep, 0)) cells leave, the h smallest under (key, item).  A
// SELECT pass finds the cut tau = the h-th smallest pair, an exclusive scan of h gives every row its place in the answer, an EMIT pass
// walks the row in its stored order, computes every key again and writes the cells at or below tau -- ascending without a sort.  No key is
// ever stored in HBM.  The selection is exact and integer throughout; it is tiered by row length:
//   * up to HO_WAVE_MAX = 256 cells: one wave holds the row in registers, four cells a lane, and descends the 96 bits of (key, item) with
//     ballots and popcounts until one candidate is left;
//   * up to HO_LDS_MAX = 4096 cells: a workgroup computes the keys once into LDS and descends eight bits at a time: an LDS histogram of
//     the digit (integer LDS atomics), a wave scan of its 256 bins, the bin that holds the rank;
//   * longer rows: the same descent with the keys computed again per level instead of stored, until the bin that holds the rank has at
//     most HO_LDS_MAX members; those are gathered into LDS and the descent finishes there.
// The first kernel visits every listed row and hands the rows of the two longer tiers to them through two lists on the device; a row's
// answer depends on its own cells only, so neither the lists' order nor the launch geometry can show in it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "philox.hpp"
#include "session_merge.hpp"

namespace {

constexpr unsigned HO_WAVE_MAX = 256;    // cells of a row one wave holds in registers: four a lane
constexpr int HO_PER_LANE = 4;
constexpr unsigned HO_LDS_MAX = 4096;    // cells whose keys and items fit a workgroup's LDS: 12 B a cell, 48 KB
constexpr int HO_LEVELS = 12;            // digits of eight bits in a (key, item) pair: eight of the key, most significant first, four of the item
constexpr int HO_GIANT_THREADS = 1024;

struct HoRule {
    unsigned n_out, min_keep;
    u64 thresh;                // 0 .. 2^32
    uint32_t seed_lo, seed_hi;
};

// key(u, j) = (w[0] << 32) | w[1] of the block at counter (j, 1, u lo, u hi) under the seed
__device__ __forceinline__ u64 ho_key(unsigned j, u64 u, const HoRule& r)
{
    const uint32_t ctr[4] = { j, 1u, (uint32_t)u, (uint32_t)(u >> 32) }, key[2] = { r.seed_lo, r.seed_hi };
    uint32_t w[4];
    pmf_philox4x32_10(ctr, key, w);
    return ((u64)w[0] << 32) | w[1];
}

__device__ __forceinline__ unsigned ho_held(unsigned len, unsigned below, const HoRule& r)
{
    const unsigned spare = len > r.min_keep ? len - r.min_keep : 0u;
    return min(min(r.n_out, below), spare);
}

struct HoSel {
    const u64* indptr;
    const unsigned* indices;
    const unsigned* rows;      // the listed rows, or nullptr: row i is listed at i
    size_t n_rows;
    HoRule r;
    u64* held;                 // [n_rows + 1]: h per listed row, and a zero behind them for the scan
    u64* tau_key;              // [n_rows]: the cut; all ones when the whole row leaves (or none: held says so)
    unsigned* tau_item;        // [n_rows]
    unsigned* list_lds;        // [n_rows]: listed rows of the LDS tier, in no order
    unsigned* list_giant;      // [n_rows]: of the longest tier
    unsigned* counts;          // [2]: how many each list holds
};

// ---- the descent by digits, on LDS -----------------------------------------------------------------------------------------------------

struct HoLds {
    u64 key[HO_LDS_MAX];
    unsigned item[HO_LDS_MAX];
    unsigned hist[256];
    unsigned sel[3];           // the picked bin, the rank inside it, its count
    unsigned word;             // a counter of the caller's
    u64 res_key;
    unsigned res_item;
};

// do the `level` most significant digits of (key, item) equal those of the prefix (pk, pi)?
__device__ __forceinline__ bool ho_match(u64 key, unsigned item, int level, u64 pk, unsigned pi)
{
    if (level == 0) return true;
    if (level < 8) return ((key ^ pk) >> (64 - 8 * level)) == 0;
    if (key != pk) return false;
    return level == 8 || ((item ^ pi) >> (32 - 8 * (level - 8))) == 0;
}
__device__ __forceinline__ unsigned ho_digit(u64 key, unsigned item, int level)
{
    return level < 8 ? (unsigned)(key >> (56 - 8 * level)) & 255u : (item >> (24 - 8 * (level - 8))) & 255u;
}
__device__ __forceinline__ void ho_extend(u64& pk, unsigned& pi, int level, unsigned bin)
{
    if (level < 8) pk |= (u64)bin << (56 - 8 * level); else pi |= bin << (24 - 8 * (level - 8));
}

// The bin of S.hist that holds the zero-based rank (the bins sum to more than rank): S.sel = { bin, rank inside it, its count }.  The first
// wave does it: four bins a lane, an inclusive scan over the lanes.  Barriers before and behind are the caller's.
__device__ __forceinline__ void ho_pick_bin(HoLds& S, unsigned rank)
{
    if (threadIdx.x >= 64) return;
    const unsigned lane = threadIdx.x;
    const unsigned c0 = S.hist[4 * lane], c1 = S.hist[4 * lane + 1], c2 = S.hist[4 * lane + 2], c3 = S.hist[4 * lane + 3];
    const unsigned own = c0 + c1 + c2 + c3;
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if (lane >= (unsigned)d) incl += t;
    }
    const unsigned excl = incl - own;
    if (excl <= rank && rank < incl) {
        unsigned r = rank - excl, b = 0, c = c0;
        if (r >= c) { r -= c; b = 1; c = c1; if (r >= c) { r -= c; b = 2; c = c2; if (r >= c) { r -= c; b = 3; c = c3; } } }
        S.sel[0] = 4 * lane + b; S.sel[1] = r; S.sel[2] = c;
    }
}

// S.key / S.item [n <= HO_LDS_MAX]: among the pairs whose `level` leading digits are the prefix (pk, pi), the one of zero-based rank `rank`
// goes to S.res_key / S.res_item.  The whole workgroup calls it; it ends behind a barrier.
__device__ void ho_lds_select(HoLds& S, unsigned n, int level, u64 pk, unsigned pi, unsigned rank)
{
    const unsigned nt = blockDim.x, tid = threadIdx.x;
    for (; level < HO_LEVELS; level++) {
        for (unsigned b = tid; b < 256; b += nt) S.hist[b] = 0u;
        __syncthreads();
        for (unsigned c = tid; c < n; c += nt)
            if (ho_match(S.key[c], S.item[c], level, pk, pi)) atomicAdd(&S.hist[ho_digit(S.key[c], S.item[c], level)], 1u);
        __syncthreads();
        ho_pick_bin(S, rank);
        __syncthreads();
        const unsigned cnt = S.sel[2];
        rank = S.sel[1];
        ho_extend(pk, pi, level, S.sel[0]);
        if (cnt == 1) {   // one pair is left: whoever holds it says what it is
            for (unsigned c = tid; c < n; c += nt)
                if (ho_match(S.key[c], S.item[c], level + 1, pk, pi)) { S.res_key = S.key[c]; S.res_item = S.item[c]; }
            __syncthreads();
            return;
        }
    }
    if (tid == 0) { S.res_key = pk; S.res_item = pi; }   // (pairs that agree in all 96 bits: a row that lists an item twice)
    __syncthreads();
}

// ---- select: the short rows, a wave each; the longer ones are handed on ----------------------------------------------------------------

__global__ __launch_bounds__(256) void holdout_select_kernel(HoSel a)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t nw = (size_t)gridDim.x * 4;
    for (size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < a.n_rows; i += nw) {
        const u64 u = a.rows != nullptr ? a.rows[i] : i;
        const u64 p0 = a.indptr[u];
        const unsigned len = (unsigned)(a.indptr[u + 1] - p0);
        if (len > HO_WAVE_MAX) {
            if (lane == 0) {
                const int giant = len > HO_LDS_MAX ? 1 : 0;
                const unsigned slot = atomicAdd(&a.counts[giant], 1u);
                (giant ? a.list_giant : a.list_lds)[slot] = (unsigned)i;
            }
            continue;
        }
        u64 key[HO_PER_LANE];
        unsigned item[HO_PER_LANE];
        bool cand[HO_PER_LANE];
        unsigned below = 0;
#pragma unroll
        for (int q = 0; q < HO_PER_LANE; q++) {
            const unsigned c = (unsigned)q * 64u + lane;
            cand[q] = c < len;
            item[q] = cand[q] ? a.indices[p0 + c] : 0u;
            key[q] = cand[q] ? ho_key(item[q], u, a.r) : 0ull;
            below += (unsigned)__popcll(__ballot(cand[q] && (key[q] >> 32) < a.r.thresh));
        }
        const unsigned h = ho_held(len, below, a.r);
        unsigned tk_hi = ~0u, tk_lo = ~0u, ti = ~0u;
        if (h > 0 && h < len) {
            // the descent: of the candidates, those with a 0 in the bit come first; the rank says which side the cut is on
            unsigned rank = h - 1, left = len;
            for (int b = 95; b >= 0 && left > 1; b--) {
                bool zero[HO_PER_LANE];
                unsigned n0 = 0;
#pragma unroll
                for (int q = 0; q < HO_PER_LANE; q++) {
                    const unsigned bit = b >= 32 ? (unsigned)(key[q] >> (b - 32)) & 1u : (item[q] >> b) & 1u;
                    zero[q] = cand[q] && bit == 0u;
                    n0 += (unsigned)__popcll(__ballot(zero[q]));
                }
                if (rank < n0) {
                    left = n0;
#pragma unroll
                    for (int q = 0; q < HO_PER_LANE; q++) cand[q] = zero[q];
                } else {
                    rank -= n0;
                    left -= n0;
#pragma unroll
                    for (int q = 0; q < HO_PER_LANE; q++) cand[q] = cand[q] && !zero[q];
                }
            }
#pragma unroll
            for (int q = 0; q < HO_PER_LANE; q++) {
                const u64 who = __ballot(cand[q]);
                if (who != 0ull) {
                    const int src = __ffsll((long long)who) - 1;
                    tk_hi = __shfl((unsigned)(key[q] >> 32), src);
                    tk_lo = __shfl((unsigned)key[q], src);
                    ti = __shfl(item[q], src);
                }
            }
        }
        if (lane == 0) { a.held[i] = h; a.tau_key[i] = ((u64)tk_hi << 32) | tk_lo; a.tau_item[i] = ti; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.held[a.n_rows] = 0ull;
}

// ---- select: rows whose keys fit LDS, a workgroup each ---------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void holdout_select_lds_kernel(HoSel a)
{
    __shared__ HoLds S;
    const unsigned tid = threadIdx.x, n_list = a.counts[0];
    for (unsigned t = blockIdx.x; t < n_list; t += gridDim.x) {
        const size_t i = a.list_lds[t];
        const u64 u = a.rows != nullptr ? a.rows[i] : i;
        const u64 p0 = a.indptr[u];
        const unsigned len = (unsigned)(a.indptr[u + 1] - p0);   // (HO_WAVE_MAX < len <= HO_LDS_MAX: the first kernel listed it here)
        if (tid == 0) S.word = 0u;
        __syncthreads();
        unsigned below = 0;
        for (unsigned c = tid; c < len; c += 256u) {
            const unsigned item = a.indices[p0 + c];
            const u64 key = ho_key(item, u, a.r);
            S.key[c] = key;
            S.item[c] = item;
            below += (key >> 32) < a.r.thresh ? 1u : 0u;
        }
        atomicAdd(&S.word, below);
        __syncthreads();
        const unsigned h = ho_held(len, S.word, a.r);
        u64 tk = ~0ull;
        unsigned ti = ~0u;
        if (h > 0 && h < len) {
            ho_lds_select(S, len, 0, 0ull, 0u, h - 1);
            tk = S.res_key;
            ti = S.res_item;
        }
        if (tid == 0) { a.held[i] = h; a.tau_key[i] = tk; a.tau_item[i] = ti; }
        __syncthreads();   // (S is the next row's)
    }
}

// ---- select: the longest rows, a workgroup each, keys computed again per level ---------------------------------------------------------

__global__ __launch_bounds__(HO_GIANT_THREADS) void holdout_select_giant_kernel(HoSel a)
{
    __shared__ HoLds S;
    const unsigned tid = threadIdx.x, n_list = a.counts[1];
    for (unsigned t = blockIdx.x; t < n_list; t += gridDim.x) {
        const size_t i = a.list_giant[t];
        const u64 u = a.rows != nullptr ? a.rows[i] : i;
        const u64 p0 = a.indptr[u];
        const unsigned len = (unsigned)(a.indptr[u + 1] - p0);
        u64 pk = 0ull, tk = ~0ull;
        unsigned pi = 0u, ti = ~0u, h = 0u, rank = 0u, cnt = len;
        int level = 0;
        for (;;) {
            for (unsigned b = tid; b < 256u; b += HO_GIANT_THREADS) S.hist[b] = 0u;
            if (tid == 0) S.word = 0u;
            __syncthreads();
            unsigned below = 0;
            for (unsigned c = tid; c < len; c += HO_GIANT_THREADS) {
                const unsigned item = a.indices[p0 + c];
                const u64 key = ho_key(item, u, a.r);
                if (ho_match(key, item, level, pk, pi)) atomicAdd(&S.hist[ho_digit(key, item, level)], 1u);
                below += (key >> 32) < a.r.thresh ? 1u : 0u;
            }
            if (level == 0) atomicAdd(&S.word, below);
            __syncthreads();
            if (level == 0) {
                h = ho_held(len, S.word, a.r);
                rank = h - 1;
                if (h == 0 || h == len) break;
            }
            ho_pick_bin(S, rank);
            __syncthreads();
            cnt = S.sel[2];
            rank = S.sel[1];
            ho_extend(pk, pi, level, S.sel[0]);
            level++;
            if (cnt <= HO_LDS_MAX || level == HO_LEVELS) break;
        }
        if (h > 0 && h < len) {
            if (level == HO_LEVELS) { tk = pk; ti = pi; }
            else {
                // the picked bin's members into LDS, in whatever order they arrive: the selection does not see it
                if (tid == 0) S.word = 0u;
                __syncthreads();
                for (unsigned c = tid; c < len; c += HO_GIANT_THREADS) {
                    const unsigned item = a.indices[p0 + c];
                    const u64 key = ho_key(item, u, a.r);
                    if (ho_match(key, item, level, pk, pi)) {
                        const unsigned slot = atomicAdd(&S.word, 1u);
                        if (slot < HO_LDS_MAX) { S.key[slot] = key; S.item[slot] = item; }
                    }
                }
                __syncthreads();
                ho_lds_select(S, min(cnt, HO_LDS_MAX), level, pk, pi, rank);
                tk = S.res_key;
                ti = S.res_item;
            }
        }
        if (tid == 0) { a.held[i] = h; a.tau_key[i] = tk; a.tau_item[i] = ti; }
        __syncthreads();
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------

template <class T> struct HoEmit {
    const u64* indptr;
    const unsigned* indices;
    const T* values;           // nullptr when only flags are asked for
    const unsigned* rows;
    size_t n_rows;
    HoRule r;
    const u64* held;           // [n_rows]
    const u64* off;            // [n_rows + 1]: its exclusive scan
    const u64* tau_key;
    const unsigned* tau_item;
    const unsigned* list_giant;
    const unsigned* counts;
    unsigned *out_row, *out_col;   // the triplets, [off[n_rows]] ...
    T* out_val;
    unsigned char* flag;           // ... or a byte per stored cell of the whole matrix, zeroed by the caller: held-out cells get a 1
};

// the stored cell at place p (item j of user u) leaves: its triplet goes to place `at` of the answer, or its flag is set
template <class T> __device__ __forceinline__ void ho_write(const HoEmit<T>& a, u64 u, u64 p, unsigned j, u64 at)
{
    if (a.flag != nullptr) { a.flag[p] = 1; return; }
    a.out_row[at] = (unsigned)u;
    a.out_col[at] = j;
    a.out_val[at] = a.values[p];
}

// A wave per listed row of the two shorter tiers: 64 cells a step in the row's stored order, a ballot prefix places the held-out ones.
// A write happens only below the row's own h, so nothing can land outside [off[i], off[i + 1]).
template <class T> __global__ __launch_bounds__(256) void holdout_emit_kernel(HoEmit<T> a)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t nw = (size_t)gridDim.x * 4;
    for (size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < a.n_rows; i += nw) {
        const unsigned h = (unsigned)a.held[i];
        if (h == 0) continue;
        const u64 u = a.rows != nullptr ? a.rows[i] : i;
        const u64 p0 = a.indptr[u];
        const unsigned len = (unsigned)(a.indptr[u + 1] - p0);
        if (len > HO_LDS_MAX) continue;   // (the workgroup kernel's)
        const u64 tk = a.tau_key[i], base = a.off[i];
        const unsigned ti = a.tau_item[i];
        unsigned done = 0;
        for (unsigned c0 = 0; c0 < len && done < h; c0 += 64u) {
            const unsigned c = c0 + lane;
            const bool live = c < len;
            const unsigned item = live ? a.indices[p0 + c] : 0u;
            const u64 key = live ? ho_key(item, u, a.r) : 0ull;
            const bool out = live && (key < tk || (key == tk && item <= ti));
            const u64 who = __ballot(out);
            const unsigned nth = done + (unsigned)__popcll(who & ((1ull << lane) - 1ull));
            if (out && nth < h) ho_write(a, u, p0 + c, item, base + nth);
            done += (unsigned)__popcll(who);
        }
    }
}

// A workgroup per row of the longest tier: 1024 cells a step, the waves' counts meet in LDS.
template <class T> __global__ __launch_bounds__(HO_GIANT_THREADS) void holdout_emit_giant_kernel(HoEmit<T> a)
{
    constexpr int NW = HO_GIANT_THREADS / 64;
    __shared__ unsigned wsum[NW];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_list = a.counts[1];
    for (unsigned t = blockIdx.x; t < n_list; t += gridDim.x) {
        const size_t i = a.list_giant[t];
        const unsigned h = (unsigned)a.held[i];
        if (h == 0) continue;
        const u64 u = a.rows != nullptr ? a.rows[i] : i;
        const u64 p0 = a.indptr[u];
        const unsigned len = (unsigned)(a.indptr[u + 1] - p0);
        const u64 tk = a.tau_key[i], base = a.off[i];
        const unsigned ti = a.tau_item[i];
        unsigned done = 0;
        for (unsigned c0 = 0; c0 < len && done < h; c0 += HO_GIANT_THREADS) {
            const unsigned c = c0 + threadIdx.x;
            const bool live = c < len;
            const unsigned item = live ? a.indices[p0 + c] : 0u;
            const u64 key = live ? ho_key(item, u, a.r) : 0ull;
            const bool out = live && (key < tk || (key == tk && item <= ti));
            const u64 who = __ballot(out);
            if (lane == 0) wsum[wave] = (unsigned)__popcll(who);
            __syncthreads();
            unsigned before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) { const unsigned n = wsum[w]; all += n; if ((unsigned)w < wave) before += n; }
            const unsigned nth = done + before + (unsigned)__popcll(who & ((1ull << lane) - 1ull));
            if (out && nth < h) ho_write(a, u, p0 + c, item, base + nth);
            done += all;
            __syncthreads();   // (wsum is the next step's)
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------

struct HoPlan {
    u64 *held = nullptr, *off = nullptr, *tau_key = nullptr;
    unsigned *tau_item = nullptr, *list_lds = nullptr, *list_giant = nullptr, *counts = nullptr;
    u64 total = 0;
};

HoRule rule_of(size_t n_out, uint64_t thresh, size_t min_keep, uint64_t seed)
{
    HoRule r;
    r.n_out = (unsigned)std::min<size_t>(n_out, 0xffffffffull);   // (a row holds fewer than 2^32 cells)
    r.min_keep = (unsigned)std::min<size_t>(min_keep, 0xffffffffull);
    r.thresh = thresh;
    r.seed_lo = (uint32_t)seed;
    r.seed_hi = (uint32_t)(seed >> 32);
    return r;
}

unsigned rows_grid(size_t n_rows) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n_rows + 3) / 4, 65536)); }

// select and scan over m > 0 listed rows (d_rows: on the device, or nullptr: all, in order): h, the cuts and the rows' places, sc's.  0 or 1.
int holdout_select(Scratch& sc, int num_cu, const u64* d_indptr, const unsigned* d_indices, const unsigned* d_rows, size_t m, const HoRule& r, HoPlan* P)
{
    const hipStream_t st = sc.stream();
    HIP_TRY(sc.get(&P->held, m + 1));
    HIP_TRY(sc.get(&P->off, m + 1));
    HIP_TRY(sc.get(&P->tau_key, m));
    HIP_TRY(sc.get(&P->tau_item, m));
    HIP_TRY(sc.get(&P->list_lds, m));
    HIP_TRY(sc.get(&P->list_giant, m));
    HIP_TRY(sc.get(&P->counts, 2));
    HIP_TRY(hipMemsetAsync(P->counts, 0, 2 * sizeof(unsigned), st));
    const HoSel a = { d_indptr, d_indices, d_rows, m, r, P->held, P->tau_key, P->tau_item, P->list_lds, P->list_giant, P->counts };
    hipLaunchKernelGGL(holdout_select_kernel, dim3(rows_grid(m)), dim3(256), 0, st, a);
    // the two lists are read on the device: the grids are sized for a full machine and a workgroup with no row ends at once
    hipLaunchKernelGGL(holdout_select_lds_kernel, dim3((unsigned)std::min<size_t>(m, (size_t)num_cu * 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(holdout_select_giant_kernel, dim3((unsigned)std::min<size_t>(m, (size_t)num_cu)), dim3(HO_GIANT_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return scan_exclusive(sc, P->held, P->off, m + 1, &P->total);
}

// the emit pass behind holdout_select: triplets (values != nullptr) or flags
void holdout_emit(hipStream_t st, int num_cu, const u64* d_indptr, const unsigned* d_indices, const real_t* d_values, const unsigned* d_rows, size_t m,
                  const HoRule& r, const HoPlan& P, unsigned* out_row, unsigned* out_col, real_t* out_val, unsigned char* flag)
{
    const HoEmit<real_t> a = { d_indptr, d_indices, d_values, d_rows, m, r, P.held, P.off, P.tau_key, P.tau_item, P.list_giant, P.counts,
                               out_row, out_col, out_val, flag };
    hipLaunchKernelGGL((holdout_emit_kernel<real_t>), dim3(rows_grid(m)), dim3(256), 0, st, a);
    hipLaunchKernelGGL((holdout_emit_giant_kernel<real_t>), dim3((unsigned)std::min<size_t>(m, (size_t)num_cu)), dim3(HO_GIANT_THREADS), 0, st, a);
}

// users (distinct, below dimA) narrowed into h32; 0 or 3
int listed_users(const sparse_ix* users, size_t n_users, size_t dimA, std::vector<unsigned>& h32)
{
    std::vector<unsigned char> mark(dimA, 0);
    h32.resize(n_users);
    for (size_t i = 0; i < n_users; i++) {
        if ((long long)users[i] < 0 || (size_t)users[i] >= dimA || mark[(size_t)users[i]]) return 3;
        mark[(size_t)users[i]] = 1;
        h32[i] = (unsigned)users[i];
    }
    return 0;
}

}  // namespace

extern "C" {

int poismf_hip_session_holdout(poismf_hip_session* s, const sparse_ix* users, size_t n_users, size_t n_out, uint64_t thresh,
                               size_t min_keep, uint64_t seed, int remove, sparse_ix* out_indptr, sparse_ix* out_indices,
                               real_t* out_values, size_t out_cap, size_t* n_held)
{
    if (n_held != nullptr) *n_held = 0;
    if (s == nullptr || out_indptr == nullptr) return 1;
    const size_t m = users == nullptr ? s->dimA : n_users;
    if (m == 0) { out_indptr[0] = 0; return 0; }
    if (thresh > (1ull << 32)) return 4;
    if (out_indices != nullptr && out_values == nullptr) return 1;
    const bool real = out_indices != nullptr;
    std::vector<unsigned> h32;
    std::vector<u64> hoff;
    try {
        if (users != nullptr) { if (const int e = listed_users(users, n_users, s->dimA, h32)) return e; }
        hoff.resize(m + 1);
    } catch (const std::bad_alloc&) { return 1; }
    pmf_last_hip_error() = hipSuccess;
    HIP_TRY(hipSetDevice(s->device));
    const Half& h = s->half[1];
    if (h.d_indptr == nullptr || h.row_begin != 0 || h.row_end != h.dimM || h.dimM != s->dimA) return 5;   // (the CSR shard must be the whole matrix)
    if (real && remove) { if (const int e = eligible(s)) return e; }
    const hipStream_t st = s->stream;
    const HoRule r = rule_of(n_out, thresh, min_keep, seed);
    Scratch sc(st);
    unsigned* d_rows = nullptr;
    if (users != nullptr) {
        HIP_TRY(sc.get(&d_rows, m));
        HIP_TRY(pmf_upload(d_rows, h32.data(), sizeof(unsigned) * m, st));
    }
    HoPlan P;
    if (holdout_select(sc, s->num_cu, h.d_indptr, h.d_indices, d_rows, m, r, &P)) return 1;
    HIP_TRY(pmf_download(hoff.data(), P.off, sizeof(u64) * (m + 1), st));
    if (sizeof(sparse_ix) < 8 && P.total > 0x7fffffffull) return 1;
    for (size_t i = 0; i <= m; i++) out_indptr[i] = (sparse_ix)hoff[i];
    if (n_held != nullptr) *n_held = (size_t)P.total;
    if (!real) return 0;
    if (P.total > out_cap) return 2;
    if (P.total == 0) return 0;
    if (P.total > 0xffffffffull) return 1;   // (the cell list of a call holds fewer than 2^32 triplets, as sub_coo's)
    const size_t total = (size_t)P.total;
    unsigned *d_row = nullptr, *d_col = nullptr;
    real_t* d_val = nullptr;
    HIP_TRY(sc.get(&d_row, total));
    HIP_TRY(sc.get(&d_col, total));
    HIP_TRY(sc.get(&d_val, total));
    holdout_emit(st, s->num_cu, h.d_indptr, h.d_indices, h.d_values, d_rows, m, r, P, d_row, d_col, d_val, nullptr);
    HIP_TRY(hipGetLastError());
    try { h32.resize(total); } catch (const std::bad_alloc&) { return 1; }
    HIP_TRY(pmf_download(h32.data(), d_col, sizeof(unsigned) * total, st));
    for (size_t e = 0; e < total; e++) out_indices[e] = (sparse_ix)h32[e];
    HIP_TRY(pmf_download(out_values, d_val, sizeof(real_t) * total, st));
    if (!remove) return 0;
    size_t removed = 0, absent = 0;
    const int rc = remove_both(s, d_row, d_col, nullptr, total, nullptr, nullptr, 0, &removed, &absent);
    return rc == 0 && removed != total ? 1 : rc;
}

int poismf_hip_holdout_mark(const sparse_ix* indptr, const sparse_ix* indices, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            size_t n_out, uint64_t thresh, size_t min_keep, uint64_t seed, unsigned char* out_flag,
                            size_t* n_held)
{
    if (n_held != nullptr) *n_held = 0;
    if (indptr == nullptr) return 1;
    const size_t m = users == nullptr ? dimA : n_users;
    if (thresh > (1ull << 32)) return 4;
    for (size_t r = 0; r < dimA; r++)
        if ((long long)indptr[r] < 0 || (long long)indptr[r + 1] < (long long)indptr[r]) return 3;
    const size_t lo = dimA ? (size_t)indptr[0] : 0, nnz = dimA ? (size_t)indptr[dimA] - lo : 0;
    if (nnz > 0xffffffffull) return 1;
    if (nnz > 0 && (indices == nullptr || out_flag == nullptr)) return 1;
    for (size_t e = 0; e < nnz; e++) {
        if ((long long)indices[lo + e] < 0 || (size_t)indices[lo + e] >= dimB) return 3;
        out_flag[e] = 0;
    }
    std::vector<unsigned> h32, hix;
    std::vector<u64> hptr;
    try {
        if (users != nullptr) { if (const int e = listed_users(users, n_users, dimA, h32)) return e; }
        if (m == 0 || nnz == 0) return 0;
        hptr.resize(dimA + 1);
        hix.resize(nnz);
    } catch (const std::bad_alloc&) { return 1; }
    for (size_t r = 0; r <= dimA; r++) hptr[r] = (u64)((size_t)indptr[r] - lo);
    for (size_t e = 0; e < nnz; e++) hix[e] = (unsigned)indices[lo + e];
    pmf_last_hip_error() = hipSuccess;
    const int device = pmf_env_device();
    HIP_TRY(hipSetDevice(device));
    int num_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, device));
    const hipStream_t st = nullptr;
    const HoRule r = rule_of(n_out, thresh, min_keep, seed);
    Scratch sc(st);
    u64* d_indptr = nullptr;
    unsigned *d_indices = nullptr, *d_rows = nullptr;
    unsigned char* d_flag = nullptr;
    HIP_TRY(sc.get(&d_indptr, dimA + 1));
    HIP_TRY(sc.get(&d_indices, nnz));
    HIP_TRY(sc.get(&d_flag, nnz));
    HIP_TRY(pmf_upload(d_indptr, hptr.data(), sizeof(u64) * (dimA + 1), st));
    HIP_TRY(pmf_upload(d_indices, hix.data(), sizeof(unsigned) * nnz, st));
    if (users != nullptr) {
        HIP_TRY(sc.get(&d_rows, m));
        HIP_TRY(pmf_upload(d_rows, h32.data(), sizeof(unsigned) * m, st));
    }
    HIP_TRY(hipMemsetAsync(d_flag, 0, nnz, st));
    HoPlan P;
    if (holdout_select(sc, std::max(num_cu, 1), d_indptr, d_indices, d_rows, m, r, &P)) return 1;
    if (P.total > 0) {
        holdout_emit(st, std::max(num_cu, 1), d_indptr, d_indices, nullptr, d_rows, m, r, P, nullptr, nullptr, nullptr, d_flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(pmf_download(out_flag, d_flag, nnz, st));
    }
    if (n_held != nullptr) *n_held = (size_t)P.total;
    return 0;
}

}  // extern "C"
