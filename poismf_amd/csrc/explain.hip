// explain.hip -- the seen items behind each recommendation (include/poismf_hip.h, section 1v): for many (user, query item) cells at
// once, the m items of the user's seen row X(u) that contribute most to the query's score, under the total order "contribution
// descending, item index ascending".
//
//   q_c    = (a_c * g_c) * b_jc                                    the query's column, rounded as written
//   d_i    = the k-ordered fused chain of a with b_i               predict's score of (u, i), bit for bit
//   num_ij = the k-ordered fused chain of b_i with q               from 0, one fma per component
//   contrib(i -> j | u) = (x_i * num_ij) / d_i                     0 where d_i is 0 or the quotient is not finite
//
// Per user this is the product  B_seen [nnz_u x k]  x  [a | q_1 .. q_T] [k x (T + 1)]:  column 0 gives every denominator from the
// tile pass that gives the numerators.  ONE WAVE owns one (user, group of up to EX_QG = 15 query items, slice of the seen row); a
// workgroup is one wave, no LDS region is shared and there is no workgroup barrier.  The wave
//   columns  builds its 16 columns [a | q] once in LDS (Qs), zero padded to a multiple of four components and in the unused columns;
//   gather   walks its slice 64 seen items at a time, lane l owning item l of the pass: the 64 rows of B go through LDS in chunks of
//            256 bytes of a row (tb_gather.hpp), the pieces of the next chunk (or pass) travelling in registers meanwhile;
//   chains   fp32: four v_mfma_f32_16x16x4_f32 row-blocks per 64 gathered rows against the 16 columns, accumulating across the
//            chunks of k -- the accumulator is the k-ordered fma chain from 0 (tb_tile.hpp); fp64: the same register layout on a
//            VALU chain (topn_batch.hip says why not the f64 MFMA);
//   epilogue hands the 16 x 64 accumulators to the lanes that own the items through LDS (the tile's own bytes, free between two
//            passes) -- so d_i and x_i are the lane's own and nothing is broadcast --, divides, applies the zero rule;
//   select   keeps a running best-m per column in LDS as (contribution, item): the pass's 64 keys and the kept m are put in order by
//            the wave's bitonic network (order_sort.hpp) in registers; a column whose kept m-th beats all 64 new keys is skipped.
// A seen row of one slice writes its cells' rows; the slices of a longer row write sorted partial rows (padded with -inf / TB_NONE)
// and explain_merge_kernel ranks them per cell (tb_merge_lists).  No m-wide row goes to device memory except those.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a
// chunk's users, query items, seen rows (host entry only: a session's rows are resident), work items, partial rows and results
// (ExLayout; poismf_hip_explain_scratch_bytes reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "order_sort.hpp"
#include "tb_batch.hpp"
#include "session.hpp"

namespace {

constexpr int EX_QG = 15;                                  // query items of a work item: with the user's own row, 16 columns
constexpr int EX_CS = 68;                                  // elements between two columns of the hand-over area [16][EX_CS]
constexpr size_t EX_M_MAX = POISMF_HIP_EXPLAIN_MAX_M;
constexpr size_t EX_Q_MAX = POISMF_HIP_EXPLAIN_MAX_QUERIES;
constexpr size_t EX_GROUPS_MAX = (EX_Q_MAX + EX_QG - 1) / EX_QG;
constexpr size_t EX_SLICE_MIN = 1024;                      // seen items per work item, unless the merge's LDS asks for more
constexpr size_t EX_MAX_ROW = POISMF_HIP_EXPLAIN_MAX_ROW;  // longest seen row of the host entry
constexpr size_t EX_PART_BYTES = (size_t)32 << 20;         // most a chunk's partial rows take, unless one user needs more
constexpr size_t EX_MORE_ITEMS = 65536;                    // work items per group beyond one per user that a chunk has room for
static_assert(EX_M_MAX <= 64, "a pass's 64 keys and the kept m are the two registers per lane of the wave's network");
static_assert(16 * EX_CS * sizeof(real_t) <= 64 * (size_t)TI_SLOT, "the hand-over area lies in the tile's bytes");
static_assert(EX_Q_MAX * TB_MERGE_MAX * (sizeof(real_t) + 4) <= EX_PART_BYTES, "one user's partial rows fit");

// chunk user, first query of the group and their number, first seen item (in sidx / sval) and their number; the row the answers go
// to: with ns == 1 the cell's own, otherwise partial row dst + t ns of column t (dst counts this slice in)
struct ExItem { unsigned long long p0; unsigned len, ui, q0, nq, dst, ns; };

struct ExArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    const unsigned* qitems;           // [chunk users][n_q] query items, TB_NONE: none
    const ExItem* items;
    const unsigned* sidx;             // seen items and counts: the chunk's rows (host entry) or the resident CSR (session)
    const real_t* sval;
    const real_t* scale;              // [k] g, or nullptr: ones
    int k;
    unsigned n_q, m;
    real_t* part_v;                   // [partial rows][m]
    unsigned* part_j;
    real_t* out_v;                    // [chunk users][n_q][m]
    unsigned* out_j;
};

// elements between two columns of Qs: k padded to a multiple of 32, plus 4 -- the MFMA's lanes (column l & 15, component l >> 4)
// then fall on distinct banks
__host__ __device__ inline size_t ex_qs(size_t k) { return ((k + 31) & ~(size_t)31) + 4; }

__host__ __device__ inline size_t ex_wave_lds(size_t k, size_t m)
{
    return (64 * (size_t)TI_SLOT + 16 * ex_qs(k) * TI_R + EX_QG * m * (TI_R + sizeof(unsigned)) + 16 * sizeof(unsigned) + 15) & ~(size_t)15;
}

// acc[t][r] += the chunk's part of the chain of column 4 (lane >> 4) + r of Qc with tile row 16 t + (lane & 15): one fused
// multiply-add per component, in ascending order.  Qc: the columns at the chunk's first component, qs elements apart.
template <class T, bool MFMA> __device__ __forceinline__ void ex_compute(T (&acc)[4][4], const T* Qc, int qs, const unsigned char* Bs, int len,
                                                                         unsigned lane)
{
    constexpr int BS = TI_SLOT / (int)sizeof(T);   // elements between two rows of the tile
    const unsigned col = lane & 15, quad = lane >> 4;
    if constexpr (MFMA) {
#if defined(__HIP_DEVICE_COMPILE__)
        // A operand: column (lane & 15) of [a | q], component 4 s + (lane >> 4); B operand: tile row (lane & 15), same component;
        // D: tile row lane & 15, column 4 (lane >> 4) + register
        const int ksteps = (len + 3) / 4;
        const float* ap = (const float*)Qc + col * qs + quad;
        const float* bp = (const float*)Bs + col * BS + quad;
        tb_f32x4 d0 = { acc[0][0], acc[0][1], acc[0][2], acc[0][3] }, d1 = { acc[1][0], acc[1][1], acc[1][2], acc[1][3] };
        tb_f32x4 d2 = { acc[2][0], acc[2][1], acc[2][2], acc[2][3] }, d3 = { acc[3][0], acc[3][1], acc[3][2], acc[3][3] };
#pragma unroll 4
        for (int s = 0; s < ksteps; s++) {
            const float av = ap[4 * s];
            const float b0 = bp[4 * s], b1 = bp[16 * BS + 4 * s], b2 = bp[32 * BS + 4 * s], b3 = bp[48 * BS + 4 * s];
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, d1, 0, 0, 0);
            d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2, d2, 0, 0, 0);
            d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3, d3, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { acc[0][r] = d0[r]; acc[1][r] = d1[r]; acc[2][r] = d2[r]; acc[3][r] = d3[r]; }
#endif
    } else {
        const T* ap = Qc + 4 * quad * qs;
        const T* bp = (const T*)Bs + col * BS;
        for (int c = 0; c < len; c++) {
            T av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) av[r] = ap[r * qs + c];
#pragma unroll
            for (int t = 0; t < 4; t++) bv[t] = bp[16 * t * BS + c];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[t][r] = ti_fma(bv[t], av[r], acc[t][r]);
        }
    }
}

template <bool MFMA> __global__ __launch_bounds__(64) void explain_kernel(ExArgs a)
{
    extern __shared__ __align__(16) unsigned char ex_smem[];
    const unsigned lane = threadIdx.x;
    const int k = a.k;
    const int qs = (int)ex_qs((size_t)k);
    const unsigned m = a.m;
    unsigned char* Bs = ex_smem;                                   // [64][TI_SLOT]: the pass's rows of B, one chunk of components
    real_t* Cs = (real_t*)ex_smem;                                 // [16][EX_CS]: a pass's chains by column, in the tile's bytes
    real_t* Qs = (real_t*)(Bs + 64 * TI_SLOT);                     // [16][qs]: a, then the group's q, zero padded
    real_t* Kv = Qs + 16 * qs;                                     // [EX_QG][m] kept contributions, best first
    unsigned* Kj = (unsigned*)(Kv + EX_QG * m);                    // [EX_QG][m] ... and their items
    unsigned* Qj = Kj + EX_QG * m;                                 // [16] the group's query items

    const ExItem it = a.items[blockIdx.x];
    const real_t* Au = a.A + (size_t)a.users[it.ui] * (size_t)k;
    if (lane < 16) Qj[lane] = lane < it.nq ? a.qitems[(size_t)it.ui * a.n_q + it.q0 + lane] : TB_NONE;
    tb_wave_sync();
    for (int c = (int)lane; c < qs; c += 64) {
        const real_t ac = c < k ? Au[c] : (real_t)0;
        const real_t ag = c < k && a.scale != nullptr ? ac * a.scale[c] : ac;
        Qs[c] = ac;
        for (int t = 0; t < EX_QG; t++) {
            const unsigned j = Qj[t];
            Qs[(t + 1) * qs + c] = c < k && j != TB_NONE ? ag * a.B[(size_t)j * (size_t)k + (size_t)c] : (real_t)0;
        }
    }
    tb_wave_sync();

    const unsigned* lst = a.sidx + it.p0;
    const real_t* cnt = a.sval + it.p0;
    const unsigned npass = (it.len + 63) / 64;
    const int nch = (k + TI_KC - 1) / TI_KC;
    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };   // (tb_gather.hpp) this lane loads piece fq + 4 g of rows frow + 16 r
    ti_u32x4 pre[TI_NI];
    unsigned j_cur = lane < it.len ? lst[lane] : TB_NONE;
    unsigned j_nxt = 64 + lane < it.len ? lst[64 + lane] : TB_NONE;
    real_t x_cur = lane < it.len ? cnt[lane] : (real_t)0;
    real_t x_nxt = 64 + lane < it.len ? cnt[64 + lane] : (real_t)0;
    real_t* brow = (real_t*)(Bs + lane * TI_SLOT);
    if (npass) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);

    unsigned kept = 0;   // entries of every column's list: min(items walked, m)
    for (unsigned pass = 0; pass < npass; pass++) {
        real_t acc[4][4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[t][r] = 0;
        for (int ch = 0; ch < nch; ch++) {
            const int c0 = ch * TI_KC;
            const int len = k - c0 < TI_KC ? k - c0 : TI_KC;
            tb_wave_sync();   // the wave is done with the tile (or the hand-over area) of the step before
            g.store(pre, j_cur, c0, len);
            for (int c = len; c < ((len + 3) & ~3); c++) brow[c] = 0;   // the MFMA reads whole groups of four components
            tb_wave_sync();
            {   // the step after this one: the next chunk of these rows, or the first chunk of the next pass's
                const bool same = ch + 1 < nch;
                const int n0 = same ? c0 + TI_KC : 0;
                if (same || pass + 1 < npass) g.fetch(pre, same ? j_cur : j_nxt, n0, k - n0 < TI_KC ? k - n0 : TI_KC);
            }
            ex_compute<real_t, MFMA>(acc, Qs + c0, qs, Bs, len, lane);
        }
        // ---- hand-over: chain (column 4 quad + r, item 16 t + col) to the lane that owns the item ----
        tb_wave_sync();
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) Cs[(4 * (lane >> 4) + r) * EX_CS + 16 * t + (lane & 15)] = acc[t][r];
        tb_wave_sync();
        const real_t d = Cs[lane];
        const unsigned left = it.len - 64 * pass;
        const unsigned seen_now = kept + (left < 64 ? left : 64u);
        const unsigned now = seen_now < m ? seen_now : m;
        for (unsigned t = 0; t < it.nq; t++) {
            real_t v = (x_cur * Cs[(t + 1) * EX_CS + lane]) / d;
            if (d == (real_t)0 || !__builtin_isfinite(v)) v = 0;
            real_t ks[2] = { j_cur != TB_NONE ? v : os_none_score(), lane < kept ? Kv[t * m + lane] : os_none_score() };
            unsigned kj[2] = { j_cur, lane < kept ? Kj[t * m + lane] : TB_NONE };
            // a full list whose last entry comes before all 64 new keys stays as it is
            if (kept == m && !__ballot(tb_better(ks[0], kj[0], Kv[t * m + m - 1], Kj[t * m + m - 1]))) continue;
            os_wave_sort<2>(ks, kj, kept ? 2u : 1u, lane);
            tb_wave_sync();   // every lane has read the list
            if (lane < now) { Kv[t * m + lane] = ks[0]; Kj[t * m + lane] = kj[0]; }
        }
        kept = now;
        j_cur = j_nxt;
        x_cur = x_nxt;
        const unsigned nx = (pass + 2) * 64 + lane;
        j_nxt = nx < it.len ? lst[nx] : TB_NONE;
        x_nxt = nx < it.len ? cnt[nx] : (real_t)0;
    }

    // ---- the slice's answer per column: the kept entries in order, the rest marked empty; a query that is none: all empty ----
    tb_wave_sync();
    for (unsigned t = 0; t < it.nq; t++) {
        const bool part = it.ns > 1;
        const size_t o = (part ? (size_t)it.dst + (size_t)t * it.ns : (size_t)it.ui * a.n_q + it.q0 + t) * m;
        const bool real = lane < kept && Qj[t] != TB_NONE;
        if (lane < m) {
            (part ? a.part_v : a.out_v)[o + lane] = real ? Kv[t * m + lane] : os_none_score();
            (part ? a.part_j : a.out_j)[o + lane] = real ? Kj[t * m + lane] : TB_NONE;
        }
    }
}

// One wave per cell of a seen row with more than one slice: mi[3 c] = its result row, mi[3 c + 1] = its first partial row, mi[3 c + 2] = its slices.
__global__ __launch_bounds__(64) void explain_merge_kernel(const real_t* part_v, const unsigned* part_j, const unsigned* mi, unsigned m, real_t* out_v,
                                                           unsigned* out_j)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX];
    const unsigned row = mi[3 * blockIdx.x], p0 = mi[3 * blockIdx.x + 1], ns = mi[3 * blockIdx.x + 2];
    real_t* o_v = out_v + (size_t)row * m;
    unsigned* o_j = out_j + (size_t)row * m;
    tb_merge_lists(ms, mj, part_v + (size_t)p0 * m, part_j + (size_t)p0 * m, ns, m, o_v, o_j);
    tb_merge_pad(mj, ns, m, o_v, o_j);   // a query that is none, or fewer than m seen items in all
}

size_t ex_slice(size_t len, size_t m)
{
    m = std::min(std::max<size_t>(m, 1), EX_M_MAX);
    const size_t most = TB_MERGE_MAX / m;   // slices of one cell the merge kernel ranks in LDS
    return pmf_round_up(std::max(EX_SLICE_MIN, pmf_ceil_div(len, most)), 64);
}
size_t ex_slices(size_t len, size_t m) { return std::max<size_t>(pmf_ceil_div(len, ex_slice(len, m)), 1); }

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.  n_cells: the seen items of the
// batch's users; `resident`: they stay where the session has them.
struct ExLayout {
    size_t groups;           // work items per user and slice
    size_t chunk_users;      // users per chunk
    size_t seen_cap;         // seen items a chunk may carry (0: resident)
    size_t item_cap;         // work items of a chunk
    size_t part_rows;        // rows of its partial lists
    size_t users, qitems, scale, sidx, sval, items, mitems, part_v, part_j, out_v, out_j, total;
    ExLayout(size_t n_users, size_t n_q, size_t m, size_t n_cells, size_t k, bool resident)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        n_q = std::min(std::max<size_t>(n_q, 1), EX_Q_MAX);
        m = std::min(std::max<size_t>(m, 1), EX_M_MAX);
        k = std::min(std::max<size_t>(k, 1), TB_K_MAX);
        groups = pmf_ceil_div(n_q, EX_QG);
        seen_cap = resident ? 0 : std::min(EX_MAX_ROW, std::max<size_t>(n_cells, 1));
        const size_t row = m * (R + 4);
        // a row of len seen items has at most len / EX_SLICE_MIN + 1 slices; only rows longer than EX_SLICE_MIN have partial rows
        const size_t long_slices = 2 * (n_cells / EX_SLICE_MIN) + 1;
        part_rows = std::max(n_q * (TB_MERGE_MAX / m), std::min(EX_PART_BYTES / row, n_q * long_slices));
        const size_t more_items = groups * std::min(n_cells / EX_SLICE_MIN + 1, EX_MORE_ITEMS);
        const size_t fixed = k * R + seen_cap * (R + 4) + more_items * sizeof(ExItem) + part_rows * (row + 6) + 512;   // (512: alignment of the eleven parts)
        const size_t per_user = sizeof(unsigned) + n_q * sizeof(unsigned) + groups * sizeof(ExItem) + n_q * row;
        chunk_users = std::max<size_t>(std::min({ (TB_BUDGET - fixed) / per_user, TB_CHUNK_USERS_MAX, n_users }), 1);
        item_cap = chunk_users * groups + more_items;
        TbTake take;
        users = take(chunk_users * sizeof(unsigned));
        qitems = take(chunk_users * n_q * sizeof(unsigned));
        scale = take(k * R);
        sidx = take(seen_cap * sizeof(unsigned));
        sval = take(seen_cap * R);
        items = take(item_cap * sizeof(ExItem));
        mitems = take(part_rows / 2 * 3 * sizeof(unsigned));
        part_v = take(part_rows * m * R);
        part_j = take(part_rows * m * sizeof(unsigned));
        out_v = take(chunk_users * n_q * m * R);
        out_j = take(chunk_users * n_q * m * sizeof(unsigned));
        total = take.o;
    }
};

// The argument checks both entry points share: 0, or 3.  No device call.
int ex_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* items, size_t n_q, const real_t* comp_scale,
             size_t m, const sparse_ix* out_ix, const real_t* out_contrib)
{
    if (m < 1 || m > EX_M_MAX || n_q < 1 || n_q > EX_Q_MAX) return 3;
    if (k < 1 || k > TB_K_MAX || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 3;
    if (users == nullptr || items == nullptr || out_ix == nullptr || out_contrib == nullptr) return 3;
    for (size_t i = 0; i < n_users; i++)
        if ((long long)users[i] < 0 || (size_t)users[i] >= dimA) return 3;
    for (size_t i = 0; i < n_users * n_q; i++)
        if (items[i] != POISMF_HIP_TOPN_NONE && ((long long)items[i] < 0 || (size_t)items[i] >= dimB)) return 3;
    for (size_t c = 0; comp_scale != nullptr && c < k; c++)
        if (!std::isfinite(comp_scale[c]) || comp_scale[c] < 0) return 3;
    return 0;
}

// The core on device-resident factors.  Arguments already checked.  The seen rows are the host CSR (seen_indptr, seen_indices,
// seen_values: one row per user of the batch) or, with `res`, the resident CSR whose counts are res_values: rows of A.
int ex_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t k, bool compact_A, const sparse_ix* users, size_t n_users,
           const sparse_ix* items, size_t n_q, const sparse_ix* seen_indptr, const sparse_ix* seen_indices, const real_t* seen_values,
           PmfTopnSeen* res, const real_t* res_values, const real_t* comp_scale, size_t m, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix,
           real_t* out_contrib)
{
    if (res != nullptr) {
        const size_t nrows = res->row_end - res->row_begin;
        std::vector<unsigned long long>& ip = *res->h_indptr;
        if (ip.size() != nrows + 1) {
            ip.resize(nrows + 1);
            TB_TRY(pmf_download(ip.data(), res->d_indptr, (nrows + 1) * sizeof(unsigned long long), stream));
        }
    }
    auto row_p0 = [&](size_t i) {
        return res ? (size_t)(*res->h_indptr)[(size_t)users[i] - res->row_begin] : (size_t)seen_indptr[i];
    };
    auto row_len = [&](size_t i) {
        if (res == nullptr) return (size_t)seen_indptr[i + 1] - (size_t)seen_indptr[i];
        const size_t r = (size_t)users[i] - res->row_begin;
        return (size_t)((*res->h_indptr)[r + 1] - (*res->h_indptr)[r]);
    };
    size_t n_cells = 0;
    for (size_t i = 0; i < n_users; i++) n_cells += row_len(i);
    const ExLayout L(n_users, n_q, m, n_cells, k, res != nullptr);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    auto kern = explain_kernel<sizeof(real_t) == 4>;   // fp32: the MFMA chain; fp64: the VALU chain
    const size_t lds = ex_wave_lds(k, m);
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ex_wave_lds(TB_K_MAX, EX_M_MAX)));
    if (comp_scale != nullptr) TB_TRY(pmf_upload(base + L.scale, comp_scale, k * sizeof(real_t), stream));

    ExArgs a;
    a.A = dA;
    a.B = dB;
    a.users = (const unsigned*)(base + L.users);
    a.qitems = (const unsigned*)(base + L.qitems);
    a.items = (const ExItem*)(base + L.items);
    a.sidx = res ? res->d_indices : (const unsigned*)(base + L.sidx);
    a.sval = res ? res_values : (const real_t*)(base + L.sval);
    a.scale = comp_scale ? (const real_t*)(base + L.scale) : nullptr;
    a.k = (int)k;
    a.n_q = (unsigned)n_q;
    a.m = (unsigned)m;
    a.part_v = (real_t*)(base + L.part_v);
    a.part_j = (unsigned*)(base + L.part_j);
    a.out_v = (real_t*)(base + L.out_v);
    a.out_j = (unsigned*)(base + L.out_j);

    std::vector<unsigned> hu, hq, hs, hm, hix;
    std::vector<ExItem> plan;
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose seen rows, work items and partial rows fit their areas together
        size_t nu = 0, cells = 0, n_items = 0, prow = 0;
        for (; u0 + nu < n_users && nu < L.chunk_users; nu++) {
            const size_t len = row_len(u0 + nu), ns = ex_slices(len, m), pr = ns > 1 ? n_q * ns : 0;
            if (nu > 0 && ((res == nullptr && cells + len > L.seen_cap) || n_items + L.groups * ns > L.item_cap || prow + pr > L.part_rows)) break;
            cells += len;
            n_items += L.groups * ns;
            prow += pr;
        }
        if ((res == nullptr && cells > L.seen_cap) || n_items > L.item_cap || prow > L.part_rows) return 1;   // (cannot happen: ExLayout sizes the areas for any user)
        // the plan: one work item per (user, group of queries, slice)
        plan.clear();
        hm.clear();
        hu.resize(nu);
        hq.resize(nu * n_q);
        const size_t p_base = res ? 0 : row_p0(u0);
        size_t next_part = 0;
        for (size_t i = 0; i < nu; i++) {
            hu[i] = compact_A ? (unsigned)(u0 + i) : (unsigned)users[u0 + i];
            for (size_t t = 0; t < n_q; t++) {
                const sparse_ix j = items[(u0 + i) * n_q + t];
                hq[i * n_q + t] = j == POISMF_HIP_TOPN_NONE ? TB_NONE : (unsigned)j;
            }
            const size_t len = row_len(u0 + i), p0 = row_p0(u0 + i) - p_base;
            const size_t sl = ex_slice(len, m), ns = ex_slices(len, m);
            for (size_t q0 = 0; q0 < n_q; q0 += EX_QG) {
                const size_t nq = std::min<size_t>(EX_QG, n_q - q0);
                for (size_t s = 0; s < ns; s++)
                    plan.push_back({ (unsigned long long)(p0 + s * sl), (unsigned)std::min(sl, len - s * sl), (unsigned)i, (unsigned)q0, (unsigned)nq,
                                     (unsigned)(next_part + q0 * ns + s), (unsigned)ns });
                for (size_t t = 0; ns > 1 && t < nq; t++)
                    hm.insert(hm.end(), { (unsigned)(i * n_q + q0 + t), (unsigned)(next_part + (q0 + t) * ns), (unsigned)ns });
            }
            if (ns > 1) next_part += n_q * ns;
        }
        if (plan.size() != n_items || next_part != prow || hm.size() > L.part_rows / 2 * 3) return 1;   // (the cut above counted the same)
        TB_TRY(pmf_upload(base + L.users, hu.data(), nu * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.qitems, hq.data(), nu * n_q * sizeof(unsigned), stream));
        if (res == nullptr) {
            hs.resize(cells);
            for (size_t p = 0; p < cells; p++) hs[p] = (unsigned)seen_indices[p_base + p];
            TB_TRY(pmf_upload(base + L.sidx, hs.data(), cells * sizeof(unsigned), stream));
            TB_TRY(pmf_upload(base + L.sval, seen_values + p_base, cells * sizeof(real_t), stream));
        }
        TB_TRY(pmf_upload(base + L.items, plan.data(), plan.size() * sizeof(ExItem), stream));
        TB_TRY(pmf_upload(base + L.mitems, hm.data(), hm.size() * sizeof(unsigned), stream));
        hipLaunchKernelGGL(kern, dim3((unsigned)plan.size()), dim3(64), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (!hm.empty()) {
            hipLaunchKernelGGL(explain_merge_kernel, dim3((unsigned)(hm.size() / 3)), dim3(64), 0, stream, a.part_v, a.part_j,
                               (const unsigned*)(base + L.mitems), (unsigned)m, a.out_v, a.out_j);
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_q * m, a.out_j, a.out_v, hix, out_ix, out_contrib, stream)) return 1;
        u0 += nu;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t poismf_hip_explain_scratch_bytes(size_t n_users, size_t n_q, size_t m, size_t n_cells, size_t k, int resident)
{
    return ExLayout(n_users, n_q, m, n_cells, k, resident != 0).total;
}

size_t poismf_hip_explain_slice(size_t len, size_t m) { return ex_slice(len, m); }

int poismf_hip_explain(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                       const sparse_ix* items, size_t n_q, const sparse_ix* seen_indptr, const sparse_ix* seen_indices, const real_t* seen_values,
                       const real_t* comp_scale, size_t m, sparse_ix* out_ix, real_t* out_contrib)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || seen_indptr == nullptr) return 3;
    if (const int rc = ex_check(users, n_users, dimA, dimB, (size_t)k, items, n_q, comp_scale, m, out_ix, out_contrib)) return rc;
    if (!tb_rows_ok(seen_indptr, seen_indices, n_users, dimB, EX_MAX_ROW)) return 3;
    if (seen_values == nullptr && seen_indptr[n_users] > seen_indptr[0]) return 3;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return ex_run(st, dA, dB, (size_t)k, compact, users, n_users, items, n_q, seen_indptr, seen_indices, seen_values, nullptr,
                                       nullptr, comp_scale, m, d_scratch, scratch_cap, out_ix, out_contrib);
                     });
}

// Section 1v from the resident factors and the resident CSR rows: ordered after the work already enqueued on the session stream, in
// the scratch the other serving calls share; no factor and no seen row is uploaded.
int poismf_hip_session_explain(poismf_hip_session* s, const sparse_ix* users, size_t n_users, const sparse_ix* items, size_t n_q,
                               const real_t* comp_scale, size_t m, sparse_ix* out_ix, real_t* out_contrib)
{
    if (n_users == 0) return 0;
    if (s == nullptr) return 3;
    if (const int rc = ex_check(users, n_users, s->dimA, s->dimB, s->k, items, n_q, comp_scale, m, out_ix, out_contrib)) return rc;
    const Half& h = s->half[1];
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] < h.row_begin || (size_t)users[i] >= h.row_end) return 3;
    PmfTopnSeen res = { h.d_indptr, h.d_indices, h.row_begin, h.row_end, &s->topn_indptr, &s->csr_rows_sorted };
    if (hipSetDevice(s->device) != hipSuccess) return 1;
    return ex_run(s->stream, s->dA, s->dB, s->k, false, users, n_users, items, n_q, nullptr, nullptr, nullptr, &res, h.d_values, comp_scale, m,
                  &s->d_topn, &s->topn_cap, out_ix, out_contrib);
}

}  // extern "C"
