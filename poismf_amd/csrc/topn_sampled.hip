// topn_sampled.hip -- seeded Plackett-Luce pages drawn in the top-N pass (include/poismf_hip.h, section 1w): section 1f's ranked list under
//
//   key(u, j)   = score(u, j) * r(u, j)           ONE multiplication rounded to real_t, after the chain and never fused into it (ts_mul)
//   r(u, j)     = E^(-T),  E = -log1p(-V),  V = (word(u, j) + 0.5) / 2^32
//   word(u, j)  = word j & 3 of the Philox4x32-10 block with key (seed lo, seed hi) and counter (j >> 2, 1, u lo, u hi), u the row of A
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t   (tb_tile.hpp)
//
// and the total order "key descending, then item index ascending": the exponential race, whose first n_top are a draw without
// replacement with probability proportional to score^(1/T).  The walk is tb_tile.hpp's and the selection tb_select.hpp's, as in
// topn_weighted.hip (topn_sampled_tile_kernel drives tb_walk with tb_all_items and TbSelect<T, TbPrunePlain>: four waves, 64 users, one
// slice of the items).  What is new is the epilogue, which makes the factor of every cell on the fly:
//
//   blocks   The four items of one Philox block (equal j >> 2) against one user sit in four neighbouring lanes of tb_compute's layout:
//            lane l holds acc[t][r] = user 4 (l >> 4) + r against item 16 t + (l & 15), so the aligned quad of lanes q = l & 3 owns, per
//            t, four items x four users = four blocks.  Lane q computes the block of user r = q -- four blocks per lane and tile step,
//            not sixteen -- and the words go round the quad: a 4 x 4 transpose in three DPP quad_perm moves (ts_quad_transpose), after
//            which lane q holds word q of the blocks of users r = 0 .. 3, the words of its own four cells.
//   factor   ts_factor: E with a small relative error whatever V is -- a short series where V < 2^-6, log2 of 1 - V with the rounding
//            of 1 - V put back where V < 1/2, and log2 of the COMPLEMENT (2^32 - word - 0.5 = ~word + 0.5, exact) above, where 1 - V
//            would cancel -- and the power as exp2(-T e) exp2(-T log2 m) for E = m 2^e, the rounding of T e put back, so that the
//            error of r does not grow with |log2 E| (up to 33).  fp32 on v_log_f32 / v_exp_f32 / v_frexp_*; fp64 on the device
//            library's log1p, log2 and exp2 (a few ulp each).  Measured error of the keys: DESIGN.md section 4.34.
//   select   the selection sees finished keys only: its threshold, its prune and the merge of the slices' lists order them by a strict
//            total order and assume nothing else, so pruning and slicing stay exact.  TbSelect has no second
//            payload, so the scores of the n_top winners -- predict's bits -- are made afterwards by topn_sampled_score_kernel, one
//            sequential fma chain per winner.
//
// T = 0 takes the instance without the epilogue (DRAW = false): r = 1 exactly, no Philox, and the rows are section 1f's bit for bit.
// No LDS beyond the selection's.  No float atomics anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "philox.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "tb_select.hpp"

namespace {

constexpr size_t TS_TARGET_WGS = 768;                     // items are split over workgroups until a chunk has about this many (topn_batch.hip's target)
constexpr size_t TS_MAX_ITEMS = POISMF_HIP_TOPN_SAMPLED_MAX_ITEMS;
constexpr size_t TS_IDX_MAX = TS_MAX_ITEMS;               // exclusion indices a chunk may carry: any valid row fits (a row is shorter than dimB)
static_assert(tb_lds_bytes(TB_N_TOP_MAX + TB_ROOM, 0) <= TB_LDS_LIMIT, "the two tiles and 64 lists of the deepest n_top with TB_ROOM free slots fit LDS");
static_assert(TS_IDX_MAX * sizeof(unsigned) + (64u << 20) <= TB_BUDGET, "the budget holds a chunk's exclusion lists and 64 MiB of lists and results");

struct TsArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of the device's A
    const unsigned* ids;              // the chunk's rows of the CALLER's A: the ids of the streams (`users` itself unless the device holds the batch's rows only)
    unsigned n_users, dimB;
    int k;
    unsigned n_top, cap;              // list capacity in LDS (n_top + TB_ROOM + slack)
    unsigned nslices, tiles_per_slice;
    TbExcl excl;                      // E(u) of the chunk's users
    unsigned seed_lo, seed_hi;
    real_t temp;                      // T
    real_t* part_score;               // [n_users][nslices][n_top] keys
    unsigned* part_ix;
};

// The one rounded multiplication of section 1w (topn_weighted.hip's tw_mul, and its reasoning): the product is consumed by compares and
// stores only, and its operand is the finished chain, so nothing can contract it.  Keep it that way: no add may take this product.
__device__ __forceinline__ float ts_mul(float s, float r) { return __fmul_rn(s, r); }
__device__ __forceinline__ double ts_mul(double s, double r) { return __dmul_rn(s, r); }

// w[s] <- w[q ^ s], q = 0 .. 3 a value of the lane: two rounds of conditional swaps
__device__ __forceinline__ void ts_xor_perm(uint32_t (&w)[4], unsigned q)
{
    const bool b0 = (q & 1u) != 0, b1 = (q & 2u) != 0;
    const uint32_t a0 = b0 ? w[1] : w[0], a1 = b0 ? w[0] : w[1], a2 = b0 ? w[3] : w[2], a3 = b0 ? w[2] : w[3];
    w[0] = b1 ? a2 : a0;
    w[1] = b1 ? a3 : a1;
    w[2] = b1 ? a0 : a2;
    w[3] = b1 ? a1 : a3;
}

template <int CTRL> __device__ __forceinline__ uint32_t ts_quad_perm(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

// In: w[i] = word i of the block lane q (= lane & 3 of an aligned quad of lanes) computed.  Out: w[r] = word q of the block lane r
// computed.  Step s sends w[q ^ s] to lane q ^ s (quad_perm by xor s), where it arrives as the word of r = q ^ s.
__device__ __forceinline__ void ts_quad_transpose(uint32_t (&w)[4], unsigned q)
{
    ts_xor_perm(w, q);
    w[1] = ts_quad_perm<0xB1>(w[1]);   // quad_perm:[1,0,3,2]
    w[2] = ts_quad_perm<0x4E>(w[2]);   // quad_perm:[2,3,0,1]
    w[3] = ts_quad_perm<0x1B>(w[3]);   // quad_perm:[3,2,1,0]
    ts_xor_perm(w, q);
}

// E^(-T) for E = m 2^e: exp2(p) exp2(-T log2 m + (-T e - p)), p = -T e rounded -- the error of the exponent is that of log2 m in
// [-1, 0], not that of a number up to 33
__device__ __forceinline__ float ts_pow_neg(float E, float temp)
{
    const float m = __builtin_amdgcn_frexp_mantf(E);   // [0.5, 1)
    const float fe = (float)__builtin_amdgcn_frexp_expf(E);
    const float p = -temp * fe;
    const float pe = __builtin_fmaf(-temp, fe, -p);
    return __builtin_amdgcn_exp2f(p) * __builtin_amdgcn_exp2f(__builtin_fmaf(-temp, __builtin_amdgcn_logf(m), pe));
}
__device__ __forceinline__ double ts_pow_neg(double E, double temp)
{
    int e;
    const double m = frexp(E, &e);
    const double fe = (double)e;
    const double p = -temp * fe;
    const double pe = __builtin_fma(-temp, fe, -p);
    return exp2(p) * exp2(__builtin_fma(-temp, log2(m), pe));
}

// r = E^(-T) of a cell's word.  T <= 3 keeps it finite in fp32: E >= 2^-33, so r <= 2^99.
__device__ __forceinline__ float ts_factor(uint32_t word, float temp)
{
    constexpr float LN2 = 0.693147180559945309f;
    const bool high = word >= 0x80000000u;
    // 2^32 V, or above one half 2^32 (1 - V) = ~word + 0.5: at most 2^31, two roundings
    const float x = (float)(high ? ~word : word) + 0.5f;
    float E;
    if (high) {
        // E = -ln(1 - V) = ln 2 (32 - log2 x), x = m 2^e
        const float m = __builtin_amdgcn_frexp_mantf(x);
        const float fe = (float)(32 - __builtin_amdgcn_frexp_expf(x));
        E = LN2 * (fe - __builtin_amdgcn_logf(m));
    } else {
        const float V = x * 0x1p-32f;
        if (V < 0x1p-6f) {
            E = V * __builtin_fmaf(V, __builtin_fmaf(V, __builtin_fmaf(V, 0.25f, 0.333333343f), 0.5f), 1.0f);   // (the next term: V^4 / 5 < 2^-26)
        } else {
            // 1 - V = u + (d - V) with d = 1 - u exact: ln(1 - V) = ln u + (d - V) / u to first order in a rounding error
            const float u = 1.0f - V, d = 1.0f - u;
            E = __builtin_fmaf(-LN2, __builtin_amdgcn_logf(u), __fdividef(V - d, u));
        }
    }
    return ts_pow_neg(E, temp);
}
__device__ __forceinline__ double ts_factor(uint32_t word, double temp)
{
    const double V = ((double)word + 0.5) * 0x1p-32;   // exact
    return ts_pow_neg(-log1p(-V), temp);
}

// DRAW: the epilogue of section 1w; without it the kernel is topn_weighted_tile_kernel with every weight 1 (T = 0)
template <class T, bool MFMA, bool DRAW> __global__ __launch_bounds__(TB_WG) void topn_sampled_tile_kernel(TsArgs a)
{
    extern __shared__ __align__(16) unsigned char ts_smem[];
    T* As = (T*)ts_smem;                                  // [TB_TU][TB_KS]
    T* Bs = As + TB_TU * TB_KS;                           // [TB_TJ][TB_KS]
    const unsigned u_base = blockIdx.x * TB_TU;
    TbSelect<T, TbPrunePlain> sel;
    sel.init((unsigned char*)(Bs + TB_TJ * TB_KS), a.cap, a.n_top, TbPrunePlain(),
             [&](unsigned row) { return u_base + row < a.n_users ? a.users[u_base + row] : TB_NONE; });

    const unsigned ntiles = (a.dimB + TB_TJ - 1) / TB_TJ;
    const unsigned tile0 = blockIdx.y * a.tiles_per_slice;
    const unsigned tile1 = tile0 + a.tiles_per_slice < ntiles ? tile0 + a.tiles_per_slice : ntiles;
    const unsigned col = threadIdx.x & 15;
    auto user_row = [&](int row) { return sel.user_row(row); };
    auto pos_of = [u_base](unsigned uu) { return u_base + uu; };   // a tile row's position in the chunk

    // this lane's share of its quad's blocks: those of user r = q of its four
    const unsigned q = col & 3;
    uint32_t ctr[4] = { 0u, 1u, 0u, 0u };   // (u hi stays 0: a row of A is below 2^31)
    const uint32_t key[2] = { a.seed_lo, a.seed_hi };
    if constexpr (DRAW) {
        const unsigned pos = u_base + sel.urow0() + q;
        ctr[2] = pos < a.n_users ? a.ids[pos] : 0u;
    }

    tb_walk<T, MFMA>(As, Bs, a.A, a.B, a.k, tile0, tile1, user_row, tb_all_items(a.dimB), [&](T (&acc)[4][4], unsigned j_base) {
        // acc[t][r]: user 16 wave + 4 (lane >> 4) + r against item j_base + 16 t + col
        if constexpr (DRAW) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                uint32_t w[4];
                ctr[0] = (j_base + 16 * t + col) >> 2;   // (equal over the quad: j_base + 16 t is a multiple of four)
                pmf_philox4x32_10(ctr, key, w);
                ts_quad_transpose(w, q);                 // w[r]: word j & 3 of the block of (item j >> 2, user r)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[t][r] = ts_mul(acc[t][r], ts_factor(w[r], a.temp));
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const unsigned j = j_base + 16 * t + col;
            sel.pass(acc[t], j, j < a.dimB, a.excl, pos_of);
        }
    });
    sel.finish(a.part_score, a.part_ix, a.nslices, blockIdx.y, pos_of);   // (the best min(count, n_top), the rest marked empty)
}

// one fused multiply-add rounded once in the operands' own type (tb_gather.hpp's ti_fma): the double builtin on floats would round twice
__device__ __forceinline__ float ts_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ts_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// score[i][q] = predict's bits for (users[i], ix[i][q]): the sequential fused chain, what tb_compute gives bit for bit; -inf for an
// empty entry.  One thread per entry: n_users x n_top of them, next to n_users x dimB cells of the tile kernel.
__global__ __launch_bounds__(256) void topn_sampled_score_kernel(const real_t* A, const real_t* B, const unsigned* users, const unsigned* ix,
                                                                 unsigned n_users, unsigned n_top, int k, real_t* score)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)n_users * n_top) return;
    const unsigned j = ix[i];
    real_t s = -std::numeric_limits<real_t>::infinity();
    if (j != TB_NONE) {
        const real_t* p = A + (size_t)users[i / n_top] * (size_t)k;
        const real_t* b = B + (size_t)j * (size_t)k;
        s = 0;
        for (int c = 0; c < k; c++) s = ts_fma(p[c], b[c], s);
    }
    score[i] = s;
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start (topn_weighted.hip's TwLayout without the
// weights, with the stream ids and the winners' scores).
struct TsLayout {
    size_t chunk_users;      // users per chunk
    size_t idx_cap;          // exclusion indices a chunk may carry
    size_t part_entries;     // (user, slice, rank) entries of the partial lists
    size_t users, ids, ex_indptr, ex_indices, part_score, part_ix, out_key, out_ix, out_score, total;
    // (user, slice) lists of a chunk of uc users: a slice per item tile at most and no more than the merge ranks in LDS; users x slices
    // <= TB_TU x (TS_TARGET_WGS + tiles)  (tb_slices)
    static size_t rows(size_t uc, size_t per_user_max) { return std::min(uc * per_user_max, TB_TU * TS_TARGET_WGS + TB_TU + uc); }
    TsLayout(size_t n_users, size_t n_top, size_t dimB)
    {
        const size_t R = sizeof(real_t), E = R + sizeof(unsigned);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), TS_MAX_ITEMS);
        const size_t slices_max = std::min(pmf_ceil_div(dimB, TB_TJ), std::max<size_t>(1, TB_MERGE_MAX / n_top));
        const size_t rest = TB_BUDGET - TS_IDX_MAX * sizeof(unsigned) - 512;   // (512: alignment of the nine parts)
        // per user: row of A, id, row pointer; the results (key, item, score); its lists under either bound of rows()
        const size_t own = 12 + n_top * (E + R);
        const size_t uc_a = rest / (own + slices_max * n_top * E);
        const size_t fixed = (TB_TU * TS_TARGET_WGS + TB_TU) * n_top * E;
        const size_t uc_b = rest > fixed ? (rest - fixed) / (own + n_top * E) : 0;
        size_t uc = std::min(std::max(uc_a, uc_b), TB_CHUNK_USERS_MAX);
        uc -= uc % TB_TU;                                                      // (>= TB_TU: uc_a is thousands at the deepest n_top in double)
        uc = std::min(uc, n_users);
        chunk_users = uc;
        idx_cap = std::min(TS_IDX_MAX, uc * dimB);                             // (no overflow: 2^18 x 2^24)
        part_entries = rows(uc, slices_max) * n_top;
        TbTake take;
        users = take(uc * sizeof(unsigned));
        ids = take(uc * sizeof(unsigned));
        ex_indptr = take((uc + 1) * sizeof(unsigned));
        ex_indices = take(idx_cap * sizeof(unsigned));
        part_score = take(part_entries * R);
        part_ix = take(part_entries * sizeof(unsigned));
        out_key = take(uc * n_top * R);
        out_ix = take(uc * n_top * sizeof(unsigned));
        out_score = take(uc * n_top * R);
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_sampled_scratch_bytes(size_t n_users, size_t n_top, size_t dimB, size_t k)
{
    (void)k;          // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TsLayout(n_users, n_top, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_sampled_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k, double temperature,
                                  const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (!(temperature >= 0.0 && temperature <= POISMF_HIP_TOPN_SAMPLED_MAX_T)) return 2;   // (NaN fails both)
    if (k < 1 || k > TB_K_MAX || dimB < 1 || dimB > TS_MAX_ITEMS || dimA > 0x7fffffffull) return 2;
    if (users == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TS_IDX_MAX)) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_sampled_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, double temperature, uint64_t seed, PmfTopnSeen* seen,
                                const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap,
                                sparse_ix* out_ix, real_t* out_score, real_t* out_key)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const TsLayout L(n_users, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t cap = tb_select_cap(n_top, 0);
    const size_t lds = tb_lds_bytes(cap, 0);
    if (lds > TB_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the deepest n_top)
    const bool draw = temperature != 0.0;
    auto kern = draw ? topn_sampled_tile_kernel<real_t, sizeof(real_t) == 4, true> : topn_sampled_tile_kernel<real_t, sizeof(real_t) == 4, false>;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_LDS_LIMIT));

    TsArgs a;
    std::vector<unsigned> hu, hp, hx, hix, hid;
    real_t* const d_key = (real_t*)(base + L.out_key);
    unsigned* const d_ix = (unsigned*)(base + L.out_ix);
    real_t* const d_score = (real_t*)(base + L.out_score);
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose exclusion lists fit the index area together
        // (a row is no longer than dimB, and the area holds min(TS_IDX_MAX, chunk x dimB): every row fits)
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.idx_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L),
                           hu, hp, hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        a.users = (const unsigned*)(base + L.users);
        a.ids = a.users;
        if (draw && compact_A) {   // the device's rows are the batch's positions: the streams are named by the caller's rows
            hid.resize(nu);
            for (size_t i = 0; i < nu; i++) hid[i] = (unsigned)users[u0 + i];
            TB_TRY(pmf_upload(base + L.ids, hid.data(), nu * sizeof(unsigned), stream));
            a.ids = (const unsigned*)(base + L.ids);
        }
        const size_t tiles = pmf_ceil_div(nu, TB_TU);
        const TbSlices sl = tb_slices(tiles, dimB, TS_TARGET_WGS, std::max<size_t>(1, TB_MERGE_MAX / n_top));   // (the merge kernel's LDS bounds them)
        const size_t nslices = sl.nslices;
        if (nu * nslices * n_top > L.part_entries) return 1;   // (cannot happen: TsLayout sizes the lists for any slicing of a chunk)
        a.A = dA;
        a.B = dB;
        a.n_users = (unsigned)nu;
        a.dimB = (unsigned)dimB;
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.cap = (unsigned)cap;
        a.nslices = (unsigned)nslices;
        a.tiles_per_slice = (unsigned)sl.tiles_per_slice;
        a.seed_lo = (unsigned)(seed & 0xffffffffull);
        a.seed_hi = (unsigned)(seed >> 32);
        a.temp = (real_t)temperature;
        // (one slice: its sorted, padded lists are the results)
        a.part_score = nslices == 1 ? d_key : (real_t*)(base + L.part_score);
        a.part_ix = nslices == 1 ? d_ix : (unsigned*)(base + L.part_ix);
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)nslices), dim3(TB_WG), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (nslices > 1) {
            // the lists hold finished keys: the plain merge, padding the ranks a short row does not reach
            hipLaunchKernelGGL(topn_merge_kernel<true>, dim3((unsigned)nu), dim3(64), 0, stream, a.part_score, a.part_ix, (unsigned)nu,
                               (unsigned)nslices, (unsigned)n_top, d_key, d_ix);
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, d_ix, d_key, hix, out_ix, out_key, stream)) return 1;
        if (out_score != nullptr) {
            // T = 0: the keys are the scores.  Otherwise the winners' scores are made now
            if (draw) {
                hipLaunchKernelGGL(topn_sampled_score_kernel, dim3((unsigned)pmf_ceil_div(nu * n_top, 256)), dim3(256), 0, stream, dA, dB, a.users, d_ix,
                                   (unsigned)nu, (unsigned)n_top, (int)k, d_score);
                TB_TRY(hipGetLastError());
            }
            TB_TRY(pmf_download(out_score + u0 * n_top, draw ? d_score : d_key, nu * n_top * sizeof(real_t), stream));
        }
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_sampled(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            size_t n_top, double temperature, uint64_t seed, const sparse_ix* excl_indptr, const sparse_ix* excl_indices,
                            sparse_ix* out_ix, real_t* out_score, real_t* out_key)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_sampled_check(users, n_users, n_top, dimA, dimB, (size_t)k, temperature, excl_indptr, excl_indices)) return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_sampled_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, temperature, seed, nullptr,
                                                            excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score, out_key);
                     });
}

}  // extern "C"
