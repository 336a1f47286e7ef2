// topn_include.hip -- batched top-N over per-user candidate lists (include/poismf_hip.h, section 1h): for many users at once, the n_top
// best items of each AMONG AN INCLUDE LIST OF ITS OWN, minus per-user exclusion sets, under the total order "score descending, item
// index ascending".  Only the listed rows of B are read: a ragged row gather with the selection fused behind it.
//
//   score(u, j) = the k-ordered fused chain  s = 0; for c in 0..k-1: s = fma(A[u,c], B[j,c], s)  in real_t
//
// bit for bit what pair_dot_kernel (serve.hip) and topn_tile_kernel (topn_batch.hip) compute.
//
// Work items are planned on the host, which has the row pointers: a user's list is cut into slices of poismf_hip_topn_include_slice()
// candidates and ONE WAVE owns one (user, slice); four such waves share a workgroup and nothing else -- no workgroup barrier, every
// LDS region belongs to one wave.  The wave walks its slice 64 candidates at a time, lane l owning candidate l of the pass:
//   gather   (tb_gather.hpp, shared with rank_include.hip) the 64 rows of B go through LDS in chunks of 256 bytes of a row.  All lanes load aligned 16-byte pieces, four
//            neighbouring lanes one row's 64 consecutive bytes; rows start on sizeof(real_t) only, so a row's first and last piece
//            carry up to 12 bytes of its neighbours (allocations of B carry 16 bytes of slack), which the copy into LDS drops:
//            element by element to the row's own slot, 68 dwords apart, where each lane then reads its row 16 bytes at a time
//            without bank conflicts.  The pieces of the next chunk (or pass) travel in registers while this one is multiplied.
//            (-DTI_STREAM builds the other form instead, each lane reading its own row from global memory: DESIGN.md 4.13 has both.)
//   chain    s = fma(A[u,c], B[j,c], s), A[u] broadcast from LDS.
//   select   a score that beats the wave's threshold (the n_top-th best so far) is looked up in E(u) (tb_excluded) and appended to
//            the wave's candidate list in LDS through an LDS counter; n_top + 64 slots, pruned by rank counting (tb_prune) whenever a
//            pass leaves fewer than 64 free.  Ranks under a strict total order do not depend on arrival order: no float atomics.
// A user with one slice writes its result row; the slices of the others write sorted partial lists (padded with -inf / TB_NONE) and
// topn_merge_ragged_kernel ranks them per user (tb_merge_lists) and pads what no real entry reaches.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a
// chunk's users, lists, work items, partial lists and results (TiLayout; poismf_hip_topn_include_scratch_bytes reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int TI_WAVES = 4;                               // work items per workgroup
constexpr unsigned TI_CAP = (unsigned)TB_N_TOP_MAX + 64;  // slots of a wave's candidate list: a pass can add 64
constexpr size_t TI_SLICE_MIN = 1024;                     // candidates per work item, unless the merge's LDS asks for more
constexpr size_t TI_MAX_ROW = POISMF_HIP_TOPN_INCLUDE_MAX_ROW;
constexpr size_t TI_PART_BYTES = (size_t)16 << 20;        // most a chunk's partial lists take
constexpr unsigned TI_PART = 0x80000000u;                 // TiItem::dst: a row of the partial lists, not of the results
static_assert(TI_CAP <= (unsigned)TB_PRUNE_Q * 64, "a prune keeps a whole list in TB_PRUNE_Q registers per lane");
static_assert(TI_MAX_ROW * sizeof(unsigned) == TB_BUDGET / 4, "the longest include row fills a quarter of the scratch");

struct TiItem { unsigned ui, p0, len, dst; };             // chunk user, first candidate in the chunk's index area, candidates, result row

struct TiArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    const TiItem* items;
    unsigned n_items;
    const unsigned* incl;             // the chunk's include lists, one after the other
    int k;
    unsigned n_top;
    TbExcl excl;                      // E(u) of the chunk's users
    real_t* part_score;               // [partial rows][n_top]
    unsigned* part_ix;
    real_t* out_score;                // [chunk users][n_top]
    unsigned* out_ix;
};

__host__ __device__ inline size_t ti_wave_lds(size_t k)
{
    const size_t ka = (k + 3) & ~(size_t)3;
    return (64 * (size_t)TI_SLOT + (ka + TI_CAP + 1) * TI_R + (TI_CAP + 2) * sizeof(unsigned) + 15) & ~(size_t)15;
}

template <bool STREAM> __global__ __launch_bounds__(64 * TI_WAVES) void topn_include_kernel(TiArgs a)
{
    extern __shared__ __align__(16) unsigned char ti_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned item = blockIdx.x * TI_WAVES + wave;
    if (item >= a.n_items) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.k;
    const int ka = (k + 3) & ~3;
    unsigned char* Bs = ti_smem + wave * ti_wave_lds((size_t)k);   // [64][TI_SLOT]: the pass's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                     // [ka] the user's row, zero padded
    real_t* Ls = As + ka;                                          // [TI_CAP] candidate scores
    real_t* thr_s = Ls + TI_CAP;                                   // threshold: score ...
    unsigned* Li = (unsigned*)(thr_s + 1);                         // [TI_CAP] candidate items
    unsigned* thr_j = Li + TI_CAP;                                 // ... and item
    unsigned* cnt = thr_j + 1;                                     // entries in the list

    const TiItem it = a.items[item];
    const unsigned arow = a.users[it.ui];
    const real_t* Au = a.A + (size_t)arow * (size_t)k;
    for (int c = (int)lane; c < ka; c += 64) As[c] = c < k ? Au[c] : (real_t)0;
    // the threshold starts as the empty entry (-inf, TB_NONE): every real (s, j), a score of -inf included, beats it
    if (lane == 0) { *thr_s = -std::numeric_limits<real_t>::infinity(); *thr_j = TB_NONE; *cnt = 0; }
    tb_wave_sync();

    const unsigned* lst = a.incl + it.p0;
    const unsigned npass = (it.len + 63) / 64;
    const int nch = (k + TI_KC - 1) / TI_KC;
    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };   // (tb_gather.hpp) this lane loads piece fq + 4 g of rows frow + 16 r
    ti_u32x4 pre[TI_NI];

    real_t thr = -std::numeric_limits<real_t>::infinity();
    unsigned thj = TB_NONE;
    unsigned j_cur = lane < it.len ? lst[lane] : TB_NONE;
    unsigned j_nxt = 64 + lane < it.len ? lst[64 + lane] : TB_NONE;
    const real_t* brow = (const real_t*)(Bs + lane * TI_SLOT);
    if (!STREAM && npass) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);

    for (unsigned pass = 0; pass < npass; pass++) {
        real_t s = 0;
        if (STREAM) {
            if (j_cur != TB_NONE) {
                const real_t* bj = a.B + (size_t)j_cur * (size_t)k;
                for (int c = 0; c < k; c++) s = ti_fma(As[c], bj[c], s);
            }
        } else {
            for (int ch = 0; ch < nch; ch++) {
                const int c0 = ch * TI_KC;
                const int len = k - c0 < TI_KC ? k - c0 : TI_KC;
                tb_wave_sync();   // the wave is done with the tile of the step before
                g.store(pre, j_cur, c0, len);
                tb_wave_sync();
                {   // the step after this one: the next chunk of these rows, or the first chunk of the next pass's
                    const bool same = ch + 1 < nch;
                    const int n0 = same ? c0 + TI_KC : 0;
                    if (same || pass + 1 < npass) g.fetch(pre, same ? j_cur : j_nxt, n0, k - n0 < TI_KC ? k - n0 : TI_KC);
                }
                if (j_cur != TB_NONE) {
                    int c = 0;
                    for (; c + TI_VN <= len; c += TI_VN) {
                        const ti_vec av = *(const ti_vec*)(As + c0 + c);
                        const ti_vec bv = *(const ti_vec*)(brow + c);
#pragma unroll
                        for (int e = 0; e < TI_VN; e++) s = ti_fma(av[e], bv[e], s);
                    }
                    for (; c < len; c++) s = ti_fma(As[c0 + c], brow[c], s);
                }
            }
        }
        // ---- selection: the list has room for 64 more ----
        bool appended = false;
        if (j_cur != TB_NONE && s >= thr && (s > thr || j_cur < thj) && !tb_excluded(a.excl, it.ui, arow, j_cur)) {
            const unsigned pos = atomicAdd(cnt, 1u);   // (LDS, integer)
            Ls[pos] = s;
            Li[pos] = j_cur;
            appended = true;
        }
        if (__ballot(appended)) {
            tb_wave_sync();
            const unsigned c = *cnt;
            if (c > a.n_top) {   // (fewer than 64 slots left)
                tb_prune(Ls, Li, c, a.n_top, cnt, thr_s, thr_j);
                thr = *thr_s;
                thj = *thr_j;
            }
        }
        j_cur = j_nxt;
        const unsigned nx = (pass + 2) * 64 + lane;
        j_nxt = nx < it.len ? lst[nx] : TB_NONE;
    }

    // ---- the slice's answer: the best min(count, n_top) in order, the rest marked empty ----
    tb_wave_sync();
    tb_prune(Ls, Li, *cnt, a.n_top, cnt, thr_s, thr_j);
    const unsigned c = *cnt;
    const bool part = (it.dst & TI_PART) != 0;
    const size_t o = (size_t)(it.dst & ~TI_PART) * a.n_top;
    real_t* o_score = (part ? a.part_score : a.out_score) + o;
    unsigned* o_ix = (part ? a.part_ix : a.out_ix) + o;
    for (unsigned i = lane; i < a.n_top; i += 64) {
        o_score[i] = i < c ? Ls[i] : -std::numeric_limits<real_t>::infinity();
        o_ix[i] = i < c ? Li[i] : TB_NONE;
    }
}

// One wave per user with more than one slice: mi[3 u] = its result row, mi[3 u + 1] = its first partial row, mi[3 u + 2] = its slices.
__global__ __launch_bounds__(64) void topn_merge_ragged_kernel(const real_t* part_score, const unsigned* part_ix, const unsigned* mi, unsigned n_top,
                                                               real_t* out_score, unsigned* out_ix)
{
    __shared__ real_t ms[TB_MERGE_MAX];
    __shared__ unsigned mj[TB_MERGE_MAX];
    const unsigned row = mi[3 * blockIdx.x], p0 = mi[3 * blockIdx.x + 1], ns = mi[3 * blockIdx.x + 2];
    real_t* o_score = out_score + (size_t)row * n_top;
    unsigned* o_ix = out_ix + (size_t)row * n_top;
    tb_merge_lists(ms, mj, part_score + (size_t)p0 * n_top, part_ix + (size_t)p0 * n_top, ns, n_top, o_score, o_ix);
    tb_merge_pad(mj, ns, n_top, o_score, o_ix);   // a short row: ranks that no real entry reached
}

size_t ti_slice(size_t len, size_t n_top)
{
    n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
    const size_t most = TB_MERGE_MAX / n_top;   // slices of one user the merge kernel ranks in LDS
    return pmf_round_up(std::max(TI_SLICE_MIN, pmf_ceil_div(len, most)), 64);
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct TiLayout {
    size_t chunk_users;      // users per chunk
    size_t incl_cap;         // include indices a chunk may carry
    size_t excl_cap;         // exclusion indices a chunk may carry
    size_t item_cap;         // work items of a chunk
    size_t part_rows;        // rows of its partial lists
    size_t users, ex_indptr, ex_indices, incl, items, mitems, part_score, part_ix, out_score, out_ix, total;
    TiLayout(size_t n_users, size_t n_cells, size_t n_top, size_t dimB)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        n_top = std::min(std::max<size_t>(n_top, 1), TB_N_TOP_MAX);
        dimB = std::max<size_t>(dimB, 1);
        const size_t first = std::min(n_users, TB_CHUNK_USERS_MAX);
        incl_cap = std::min(TI_MAX_ROW, std::max<size_t>(n_cells, 1));                    // a quarter of the budget at most
        excl_cap = std::min(TB_BUDGET / 2 / sizeof(unsigned), first * dimB);              // section 1f's: half of it  (no overflow: 2^18 x 2^31)
        const size_t rest = TB_BUDGET - (incl_cap + excl_cap) * sizeof(unsigned) - 512;   // (512: alignment of the ten parts)
        const size_t row = n_top * (R + 4);
        // a list of len candidates has at most len / TI_SLICE_MIN + 1 slices; only lists longer than TI_SLICE_MIN have partial rows
        part_rows = std::max(TB_MERGE_MAX / n_top, std::min(TI_PART_BYTES / row, 2 * incl_cap / TI_SLICE_MIN + 1));
        const size_t more_items = incl_cap / TI_SLICE_MIN + 1;
        const size_t fixed = part_rows * row + more_items * sizeof(TiItem);
        const size_t per_user = 2 * sizeof(unsigned) + 3 * sizeof(unsigned) + sizeof(TiItem) + row;
        chunk_users = std::max<size_t>(std::min({ (rest - fixed) / per_user, TB_CHUNK_USERS_MAX, n_users }), 1);
        item_cap = chunk_users + more_items;
        TbTake take;
        users = take(chunk_users * sizeof(unsigned));
        ex_indptr = take((chunk_users + 1) * sizeof(unsigned));
        ex_indices = take(excl_cap * sizeof(unsigned));
        incl = take(incl_cap * sizeof(unsigned));
        items = take(item_cap * sizeof(TiItem));
        mitems = take(chunk_users * 3 * sizeof(unsigned));
        part_score = take(part_rows * n_top * R);
        part_ix = take(part_rows * n_top * sizeof(unsigned));
        out_score = take(chunk_users * n_top * R);
        out_ix = take(chunk_users * n_top * sizeof(unsigned));
        total = take.o;
    }
};

}  // namespace

extern "C" size_t poismf_hip_topn_include_scratch_bytes(size_t n_users, size_t n_cells, size_t n_top, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return TiLayout(n_users, n_cells, n_top, dimB).total;
}

extern "C" size_t poismf_hip_topn_include_slice(size_t len, size_t n_top) { return ti_slice(len, n_top); }

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_topn_include_check(const sparse_ix* users, size_t n_users, size_t n_top, size_t dimA, size_t dimB, size_t k,
                                  const sparse_ix* incl_indptr, const sparse_ix* incl_indices, const sparse_ix* excl_indptr,
                                  const sparse_ix* excl_indices)
{
    if (n_top == 0 || n_top > TB_N_TOP_MAX) return 2;
    if (k < 1 || k > TB_K_MAX || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || incl_indptr == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (!tb_rows_ok(incl_indptr, incl_indices, n_users, dimB, TI_MAX_ROW)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_topn_include_run(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                const sparse_ix* users, size_t n_users, size_t n_top, const sparse_ix* incl_indptr,
                                const sparse_ix* incl_indices, PmfTopnSeen* seen, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, void** d_scratch, size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t n_cells = (size_t)incl_indptr[n_users] - (size_t)incl_indptr[0];
    const TiLayout L(n_users, n_cells, n_top, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

#ifdef TI_STREAM
    auto kern = topn_include_kernel<true>;
#else
    auto kern = topn_include_kernel<false>;
#endif
    const size_t lds = TI_WAVES * ti_wave_lds(k);
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(TI_WAVES * ti_wave_lds(TB_K_MAX))));

    TiArgs a;
    std::vector<unsigned> hu, hp, hx, hi, hm, hix;
    std::vector<TiItem> items;
    auto row_len = [](const sparse_ix* indptr, size_t i) { return indptr ? (size_t)indptr[i + 1] - (size_t)indptr[i] : 0; };
    auto slices_of = [&](size_t len) { return std::max<size_t>(pmf_ceil_div(len, ti_slice(len, n_top)), 1); };
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose include lists, exclusion lists and partial lists fit their areas together.  `fit`: how
        // many the include lists and the partial lists let in; the exclusion lists may cut the chunk shorter
        size_t fit = 0;
        for (size_t ni = 0, prow = 0; u0 + fit < n_users && fit < L.chunk_users; fit++) {
            const size_t len_i = row_len(incl_indptr, u0 + fit);
            const size_t ns = slices_of(len_i), pr = ns > 1 ? ns : 0;
            if (fit > 0 && (ni + len_i > L.incl_cap || prow + pr > L.part_rows)) break;
            ni += len_i;
            prow += pr;
        }
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, fit, L.excl_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L), hu, hp, hx,
                           stream))
            return 1;
        const size_t nu = u1 - u0, ni = (size_t)incl_indptr[u1] - (size_t)incl_indptr[u0];
        // the plan: one work item per (user, slice)
        items.clear();
        hm.clear();
        const size_t i_base = (size_t)incl_indptr[u0];
        size_t next_part = 0;
        for (size_t i = 0; i < nu; i++) {
            const size_t len = row_len(incl_indptr, u0 + i), p0 = (size_t)incl_indptr[u0 + i] - i_base;
            const size_t sl = ti_slice(len, n_top), ns = slices_of(len);
            if (ns == 1) {
                items.push_back({ (unsigned)i, (unsigned)p0, (unsigned)len, (unsigned)i });
                continue;
            }
            hm.insert(hm.end(), { (unsigned)i, (unsigned)next_part, (unsigned)ns });
            for (size_t s = 0; s < ns; s++)
                items.push_back({ (unsigned)i, (unsigned)(p0 + s * sl), (unsigned)std::min(sl, len - s * sl), TI_PART | (unsigned)(next_part + s) });
            next_part += ns;
        }
        if (items.size() > L.item_cap || next_part > L.part_rows || ni > L.incl_cap) return 1;   // (cannot happen: TiLayout sizes the areas for any chunk)
        hi.resize(ni);
        for (size_t p = 0; p < ni; p++) hi[p] = (unsigned)incl_indices[i_base + p];
        TB_TRY(pmf_upload(base + L.incl, hi.data(), ni * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.items, items.data(), items.size() * sizeof(TiItem), stream));
        TB_TRY(pmf_upload(base + L.mitems, hm.data(), hm.size() * sizeof(unsigned), stream));
        a.A = dA;
        a.B = dB;
        a.users = (const unsigned*)(base + L.users);
        a.items = (const TiItem*)(base + L.items);
        a.n_items = (unsigned)items.size();
        a.incl = (const unsigned*)(base + L.incl);
        a.k = (int)k;
        a.n_top = (unsigned)n_top;
        a.part_score = (real_t*)(base + L.part_score);
        a.part_ix = (unsigned*)(base + L.part_ix);
        a.out_score = (real_t*)(base + L.out_score);
        a.out_ix = (unsigned*)(base + L.out_ix);
        hipLaunchKernelGGL(kern, dim3((unsigned)pmf_ceil_div(items.size(), TI_WAVES)), dim3(64 * TI_WAVES), lds, stream, a);
        TB_TRY(hipGetLastError());
        if (!hm.empty()) {
            hipLaunchKernelGGL(topn_merge_ragged_kernel, dim3((unsigned)(hm.size() / 3)), dim3(64), 0, stream, a.part_score, a.part_ix,
                               (const unsigned*)(base + L.mitems), (unsigned)n_top, a.out_score, a.out_ix);
            TB_TRY(hipGetLastError());
        }
        if (tb_fetch_results(u0, nu, n_top, (const unsigned*)(base + L.out_ix), (const real_t*)(base + L.out_score), hix, out_ix, out_score, stream)) return 1;
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_topn_include(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                            size_t n_top, const sparse_ix* incl_indptr, const sparse_ix* incl_indices, const sparse_ix* excl_indptr,
                            const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_topn_include_check(users, n_users, n_top, dimA, dimB, (size_t)k, incl_indptr, incl_indices, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_topn_include_run(st, dA, dB, dimB, (size_t)k, compact, users, n_users, n_top, incl_indptr, incl_indices,
                                                            nullptr, excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score);
                     });
}

}  // extern "C"
