// topn_diverse.hip -- diversified batched top-N (include/poismf_hip.h, section 1p): greedy maximal marginal relevance over a pool of
// the best `pool` items of every user, picked on the device.
//
//   pool stage   section 1l's answer for (u, pool), left in scratch by the deep core's chunk loop (poismf_hip_topn_deep_chunks,
//                topn_deep.hip): positions 0 .. c(u) - 1 in the total order, relevance rel_i with predict_multiple's bits.
//   MMR stage    topn_diverse_mmr_kernel, below: n_top picks, each the unpicked position with the largest
//                v_i = (lam r_i) - (oml m_i),  r_i = rel_i / rel_0,  m_i = the largest cos(i, q) over the positions q picked so far,
//                cos(i, q) = ((chain(B[j_i], B[j_q]) inv[j_i]) inv[j_q]),  ties to the lowest position.
//
// ONE WAVE owns one user, four such waves share a workgroup and nothing else -- no workgroup barrier, every LDS region belongs to one
// wave.  Lane l owns pool positions l, l + 64, ...: at most TV_Q = 16 of them; lam r_i (rounded once: it never changes), m_i and the
// inverse norm of the position's item live in registers, the picked flags in a bit mask, all statically indexed through unrolled loops
// (a round of the gather names its registers by a wave-uniform compare per slot).  Per pick:
//   arg-max   every lane's best unpicked position, then a DPP reduction on (v, position) across the wave (wave_ops.hpp's moves);
//   gather    the picked row B[j_q] goes to LDS, read back at a wave-uniform address; the pool's rows of B go through tb_gather.hpp's
//             TiGather 64 at a time -- aligned 16-byte pieces, 272-byte LDS slots -- and ti_pass multiplies them, k-ordered, against the
//             picked row.  The pool is gathered again, out of the caches, on every pick: (n_top - 1) c k sizeof(real_t) bytes per user, one code
//             path for every k and pool and no LDS residency.  The first chunk of the next pick's first round
//             travels in registers across the arg-max.
//   update    the two rounded multiplications and m_i = cos > m_i ? cos : m_i.
// Nothing is contracted into an FMA outside the chain (tv_mul / tv_sub / tv_div).  No float atomics anywhere: the answer is a function
// of the pool's rows alone.
//
// The host side: the inverse norms go up once per call in front of the deep layout's parts; the picked rows (item, relevance, value)
// are three more parts of the chunk (TvLayout; poismf_hip_topn_diverse_scratch_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "wave_ops.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_batch.hpp"
#include "tb_deep.hpp"

namespace {

constexpr int TV_WAVES = 4;                               // users per workgroup
constexpr int TV_Q = (int)(TD_N_TOP_MAX / 64);            // pool positions per lane at the deepest pool
constexpr size_t TV_MAX_ITEMS = POISMF_HIP_TOPN_DIVERSE_MAX_ITEMS;
constexpr size_t TV_NORMS_MAX = TV_MAX_ITEMS * sizeof(double);   // the inverse norms at the item limit in double: 128 MiB
constexpr size_t TV_LDS_LIMIT = 96 * 1024;
static_assert(TV_Q * 64 == (int)TD_N_TOP_MAX && TV_Q <= 32, "a lane's picked flags are one bit per position in 32 bits");
static_assert(((size_t)POISMF_HIP_TOPN_DIVERSE_BUDGET_MB << 20) == TD_BUDGET + TV_NORMS_MAX, "the budget: the deep call's and the norms at their largest");

struct TvArgs {
    const real_t* B;                  // [dimB x k]
    const real_t* inv;                // [dimB] item_inv_norm
    int k;
    unsigned n_users, pool, n_top;
    real_t lam, oml;
    const unsigned* pool_ix;          // [n_users][pool] the pool stage's rows: real entries first, then TB_NONE
    const real_t* pool_score;
    unsigned* out_ix;                 // [n_users][n_top] in pick order
    real_t* out_score;
    real_t* out_value;
};

// Section 1p's operations, each rounded once.  HIP's header may define the rounded intrinsics as plain operators, and the compiler
// contracts a product INTO a subtraction that consumes it; tv_keep hands the product through an empty asm statement, which the
// contraction cannot see through and which emits nothing.  The products of the cosine are consumed by products and compares only.
__device__ __forceinline__ float tv_keep(float x) { __asm__ volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ double tv_keep(double x) { __asm__ volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float tv_mul(float a, float b) { return tv_keep(__fmul_rn(a, b)); }
__device__ __forceinline__ double tv_mul(double a, double b) { return tv_keep(__dmul_rn(a, b)); }
__device__ __forceinline__ float tv_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double tv_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float tv_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double tv_div(double a, double b) { return __ddiv_rn(a, b); }

// (v1, p1) is picked before (v2, p2): a lane with no candidate holds TB_NONE
__device__ __forceinline__ bool tv_beats(real_t v1, unsigned p1, real_t v2, unsigned p2)
{
    return p1 != TB_NONE && (p2 == TB_NONE || v1 > v2 || (v1 == v2 && p1 < p2));
}
template <int CTRL> __device__ __forceinline__ void tv_best_step(real_t& v, unsigned& p)
{
    const real_t ov = pmf::dpp_mov<CTRL>(v);
    const unsigned op = (unsigned)pmf::dpp_mov<CTRL>((int)p);
    if (tv_beats(ov, op, v, p)) { v = ov; p = op; }
}
// the wave's best (v, position), uniform: four DPP steps inside each row of 16 lanes (wave_ops.hpp's wave_reduce), then the four rows
__device__ __forceinline__ void tv_wave_best(real_t& v, unsigned& p)
{
    tv_best_step<0xB1>(v, p);
    tv_best_step<0x4E>(v, p);
    tv_best_step<0x141>(v, p);
    tv_best_step<0x140>(v, p);
    real_t bv = pmf::read_lane(v, 0);
    unsigned bp = (unsigned)pmf::read_lane((int)p, 0);
#pragma unroll
    for (int row = 1; row < 4; row++) {
        const real_t rv = pmf::read_lane(v, 16 * row);
        const unsigned rp = (unsigned)pmf::read_lane((int)p, 16 * row);
        if (tv_beats(rv, rp, bv, bp)) { bv = rv; bp = rp; }
    }
    v = pmf::uniform(bv);
    p = pmf::uniform(bp);
}

__host__ __device__ inline size_t tv_wave_lds(size_t k)
{
    const size_t ka = (k + 3) & ~(size_t)3;
    return (64 * (size_t)TI_SLOT + ka * TI_R + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(64 * TV_WAVES) void topn_diverse_mmr_kernel(TvArgs a)
{
    extern __shared__ __align__(16) unsigned char tv_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned u = blockIdx.x * TV_WAVES + wave;
    if (u >= a.n_users) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.k;
    const int ka = (k + 3) & ~3;
    unsigned char* Bs = tv_smem + wave * tv_wave_lds((size_t)k);   // [64][TI_SLOT]: a round's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                      // [ka] the picked row, zero padded
    const real_t neg_inf = -std::numeric_limits<real_t>::infinity();

    const unsigned* pix = a.pool_ix + (size_t)u * a.pool;
    const real_t* psc = a.pool_score + (size_t)u * a.pool;
    unsigned* o_ix = a.out_ix + (size_t)u * a.n_top;
    real_t* o_score = a.out_score + (size_t)u * a.n_top;
    real_t* o_value = a.out_value + (size_t)u * a.n_top;

    // c: the pool's real entries, a prefix of the row (counted as one: nothing behind the first empty entry is ever read as an item)
    unsigned c = 0;
    for (unsigned p0 = 0; p0 < a.pool; p0 += 64) {
        const unsigned long long real = __ballot(p0 + lane < a.pool && pix[p0 + lane] != TB_NONE);
        const unsigned lead = real == ~0ull ? 64u : (unsigned)__builtin_ctzll(~real);
        c += lead;
        if (lead < 64) break;
    }
    const unsigned npick = c < a.n_top ? c : a.n_top;
    for (unsigned i = npick + lane; i < a.n_top; i += 64) {
        o_ix[i] = TB_NONE;
        o_score[i] = neg_inf;
        o_value[i] = neg_inf;
    }
    if (npick == 0) return;
    const unsigned nround = (c + 63) / 64;   // <= TV_Q

    // this lane's positions qq 64 + lane: lam r, the largest cosine to a picked position, the item's inverse norm
    const real_t rel0 = psc[0];
    real_t lr[TV_Q], m[TV_Q], inv_r[TV_Q];
    unsigned picked = 0;
#pragma unroll
    for (int qq = 0; qq < TV_Q; qq++) {
        const unsigned pos = 64u * qq + lane;
        lr[qq] = 0;
        m[qq] = 0;
        inv_r[qq] = 0;
        if (pos < c) {
            const real_t rel = psc[pos];
            lr[qq] = tv_mul(a.lam, rel0 > (real_t)0 ? tv_div(rel, rel0) : rel);
            inv_r[qq] = a.inv[pix[pos]];
        }
    }

    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };   // (tb_gather.hpp) this lane loads piece fq + 4 g of rows frow + 16 r
    ti_u32x4 pre[TI_NI];
    const unsigned j_first = lane < c ? pix[lane] : TB_NONE;               // the rows of round 0
    if (npick > 1) g.fetch(pre, j_first, 0, k < TI_KC ? k : TI_KC);

    for (unsigned t = 0; t < npick; t++) {
        // ---- the pick: the unpicked position with the largest v, the lowest such position ----
        real_t bv = 0;
        unsigned bp = TB_NONE;
#pragma unroll
        for (int qq = 0; qq < TV_Q; qq++) {
            const unsigned pos = 64u * qq + lane;
            if (pos < c && !((picked >> qq) & 1u)) {
                const real_t v = tv_sub(lr[qq], tv_mul(a.oml, m[qq]));
                if (bp == TB_NONE || v > bv) { bv = v; bp = pos; }
            }
        }
        tv_wave_best(bv, bp);
        if (bp == TB_NONE) break;   // (cannot happen: fewer than c positions are picked)
        const unsigned jq = pix[bp];
        if (lane == 0) {
            o_ix[t] = jq;
            o_score[t] = psc[bp];
            o_value[t] = bv;
        }
        if (lane == (bp & 63u)) picked |= 1u << (bp >> 6);
        if (t + 1 == npick) break;

        // ---- the cosines of the pool to the picked row ----
        const bool more = t + 2 < npick;   // another update follows this one
        const real_t inv_q = a.inv[jq];
        tb_wave_sync();                    // the wave is done with the picked row of the step before
        for (int cc = (int)lane; cc < ka; cc += 64) As[cc] = cc < k ? a.B[(size_t)jq * (size_t)k + (size_t)cc] : (real_t)0;
        tb_wave_sync();
        unsigned j_cur = j_first;
        for (unsigned q = 0; q < nround; q++) {
            // the rows that follow these: the next round's, or round 0 again for the next pick's update
            const bool last = q + 1 == nround;
            const bool follow = !last || more;
            const unsigned nx = last ? lane : 64 * (q + 1) + lane;
            const unsigned j_nxt = follow && nx < c ? pix[nx] : TB_NONE;
            const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, 0u, follow ? 2u : 1u);
            real_t inv_mine = 0;
#pragma unroll
            for (int qq = 0; qq < TV_Q; qq++)
                if (qq == (int)q) inv_mine = inv_r[qq];
            const real_t cs = tv_mul(tv_mul(s, inv_mine), inv_q);
#pragma unroll
            for (int qq = 0; qq < TV_Q; qq++)
                if (qq == (int)q) m[qq] = cs > m[qq] ? cs : m[qq];
            j_cur = j_nxt;
        }
    }
}

// The one scratch allocation of a call, in bytes from the start: the inverse norms, the deep layout of the pool stage (tb_deep.hpp),
// sized so that the picked rows fit beside it, and the picked rows.
struct TvLayout {
    size_t extra_per_user, extra_fixed;   // what the deep layout leaves room for
    size_t chunk_users;
    size_t inv, deep, pick_ix, pick_score, pick_value, total;
    TvLayout(size_t n_users, size_t n_top, size_t pool, size_t dimB)
    {
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        pool = std::min(std::max(pool, n_top), TD_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), TV_MAX_ITEMS);
        extra_per_user = n_top * (sizeof(unsigned) + 2 * sizeof(real_t));
        extra_fixed = 128;                // (alignment of the deep layout and the three parts)
        const TdLayout D(n_users, pool, dimB, extra_per_user, extra_fixed);
        chunk_users = D.chunk_users;
        TbTake take;
        inv = take(dimB * sizeof(real_t));
        deep = take(D.total);
        pick_ix = take(chunk_users * n_top * sizeof(unsigned));
        pick_score = take(chunk_users * n_top * sizeof(real_t));
        pick_value = take(chunk_users * n_top * sizeof(real_t));
        total = take.o;
    }
};
static_assert(4 * (64 * (size_t)TI_SLOT + TB_K_MAX * sizeof(real_t) + 16) <= TV_LDS_LIMIT, "four waves' tiles and picked rows fit LDS at the largest k");

}  // namespace

extern "C" size_t poismf_hip_topn_diverse_scratch_bytes(size_t n_users, size_t n_top, size_t pool, size_t dimB, size_t k)
{
    (void)k;          // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TvLayout(n_users, n_top, pool, dimB).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_diverse_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t pool, double lambda, size_t dimA, size_t dimB,
                                  size_t k, const real_t* item_inv_norm, const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX || pool < n_top || pool > TD_N_TOP_MAX) return 2;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return 2;   // (NaN fails both)
    if (dimB > TV_MAX_ITEMS || item_inv_norm == nullptr) return 2;
    if (const int rc = poismf_hip_topn_deep_check(users, n_users, pool, dimA, dimB, k, excl_indptr, excl_indices)) return rc;
    for (size_t j = 0; j < dimB; j++)
        if (!std::isfinite(item_inv_norm[j]) || item_inv_norm[j] < (real_t)0) return 2;   // (-0 is 0)
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_diverse_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, size_t pool, double lambda, const real_t* item_inv_norm,
                                PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                                size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score, real_t* out_value)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const TvLayout L(n_users, n_top, pool, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t lds = TV_WAVES * tv_wave_lds(k);
    if (lds > TV_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the largest k)
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(topn_diverse_mmr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TV_LDS_LIMIT));

    TB_TRY(pmf_upload(base + L.inv, item_inv_norm, dimB * sizeof(real_t), stream));

    TvArgs a;
    a.B = dB;
    a.inv = (const real_t*)(base + L.inv);
    a.k = (int)k;
    a.pool = (unsigned)pool;
    a.n_top = (unsigned)n_top;
    a.lam = (real_t)lambda;
    a.oml = (real_t)(1.0 - lambda);
    a.out_ix = (unsigned*)(base + L.pick_ix);
    a.out_score = (real_t*)(base + L.pick_score);
    a.out_value = (real_t*)(base + L.pick_value);
    std::vector<unsigned> hix;
    return poismf_hip_topn_deep_chunks(
        stream, dA, dB, dimB, k, compact_A, users, n_users, pool, seen, excl_indptr, excl_indices, base + L.deep, L.extra_per_user, L.extra_fixed,
        [&](size_t u0, size_t nu, const unsigned* d_ix, const real_t* d_score) -> int {
            if (nu > L.chunk_users) return 1;   // (cannot happen: both layouts cut the same chunks)
            a.n_users = (unsigned)nu;
            a.pool_ix = d_ix;
            a.pool_score = d_score;
            hipLaunchKernelGGL(topn_diverse_mmr_kernel, dim3((unsigned)pmf_ceil_div(nu, TV_WAVES)), dim3(64 * TV_WAVES), lds, stream, a);
            TB_TRY(hipGetLastError());
            if (tb_fetch_results(u0, nu, n_top, a.out_ix, a.out_score, hix, out_ix, out_score, stream)) return 1;
            if (out_value != nullptr) TB_TRY(pmf_download(out_value + u0 * n_top, a.out_value, nu * n_top * sizeof(real_t), stream));
            return 0;
        });
}

extern "C" {

int poismf_hip_topn_diverse(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            size_t n_top, size_t pool, double lambda, const real_t* item_inv_norm, const sparse_ix* excl_indptr,
                            const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score, real_t* out_value)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_diverse_check(users, n_users, n_top, pool, lambda, dimA, dimB, (size_t)k, item_inv_norm, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_diverse_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, pool, lambda, item_inv_norm,
                                                            nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score, out_value);
                     });
}

}  // extern "C"
