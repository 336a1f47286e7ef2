// order_include.hip -- batched re-rank (include/poismf_hip.h, section 1s): for many users at once, each user's WHOLE candidate list,
// minus its exclusion set, in the total order "score descending, item index ascending", with the scores.  Only the listed rows of B
// are read (the ragged gather of tb_gather.hpp, whose chain is pair_dot_kernel's bit for bit); every score is kept and sorted --
// the top-N units let a score die unless it beats a threshold, this one has no threshold.
//
// The host has the row pointers and plans by row length (W = OI_WAVE_ROW, R = OI_RUN):
//   len <= W   order_wave_kernel: one wave per row, four rows per workgroup and nothing shared between them -- no workgroup barrier.
//              The wave walks the row 64 candidates per pass (ti_pass), lane l keeps the key of candidate 64 pass + l in register
//              `pass` -- an excluded candidate's key is the empty one -- and a bitonic network on lane exchanges orders the next
//              power of two of entries (os_wave_sort).  A popcount of the real keys is the row's count.
//   len <= R   order_run_kernel: one workgroup of four waves per row.  Wave w takes the passes w, w + 4, ... with a gather tile of its
//              own and writes the keys to one key array in LDS; the workgroup then holds entry 256 r + t in register r of thread t
//              and runs the network (os_wg_sort), which goes back to LDS only for the two distances that leave a wave but not a thread's
//              registers' stride.
//   len > R    the same kernel orders consecutive runs of R candidates, and order_merge_kernel merges runs pairwise, ceil(log2(runs))
//              passes between the two key areas X and Y of the scratch.  One workgroup produces OS_MERGE_BLOCK consecutive entries
//              of a merged run: it finds where the block starts and ends in both inputs by a merge-path search, loads the two
//              pieces into LDS, gives every entry its place by a search in the other piece and writes the block out in order.  A
//              row's runs start in the area from which its number of passes ends in X, where every other row is written directly:
//              X is the result.
// Empty keys are all equal and all last, the padding written is the canonical (-inf, TB_NONE), and every key has one place under a
// strict order: nothing depends on the order in which anything arrives, and there are no float atomics (a long row's count is an
// integer sum over its runs).
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds a
// chunk's users, lists, work items, both key areas and counts (OiLayout; poismf_hip_order_include_scratch_bytes reports its size).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_batch.hpp"
#include "order_sort.hpp"

namespace {

constexpr int OI_WAVES = 4;                               // waves per workgroup, both kernels
constexpr int OI_Q = 4;                                   // keys per lane of the one-wave kernel
constexpr size_t OI_WAVE_ROW = 64 * OI_Q;                 // W: longest row of the one-wave kernel
constexpr int OI_E = 8;                                   // keys per thread of the workgroup kernel at its longest row
constexpr size_t OI_RUN = (size_t)OS_WG * OI_E;           // R: entries one workgroup orders
constexpr size_t OI_MAX_ROW = POISMF_HIP_ORDER_MAX_ROW;
constexpr unsigned OI_AREA_Y = 1u;                        // OiItem::flags: the keys go to area Y, not X
constexpr unsigned OI_PART = 2u;                          // OiItem::flags: a run of a longer row: its count is added to the row's
static_assert(OS_WG == 64 * OI_WAVES, "the workgroup network's threads are the gather's four waves");
static_assert((OI_RUN & (OI_RUN - 1)) == 0 && OI_RUN >= 2048 && OI_RUN % OS_MERGE_BLOCK == 0, "runs: a power of two, whole merge blocks");
static_assert(OI_WAVE_ROW * 2 <= OI_RUN, "the workgroup network starts at 512 entries");

struct OiItem { unsigned ui, p0, len, flags; };           // chunk user, first candidate in the chunk's cell areas, candidates, OI_*
struct OmItem { unsigned p0, len, block, src; };          // row start and length, block of OS_MERGE_BLOCK entries of it, source area (1: Y)

struct OiArgs {
    const real_t* A;                  // rows addressed by `users`
    const real_t* B;                  // [dimB x k]
    const unsigned* users;            // the chunk's rows of A
    const OiItem* items;
    unsigned n_items;
    const unsigned* incl;             // the chunk's include lists, one after the other
    int k;
    TbExcl excl;                      // E(u) of the chunk's users
    real_t* xs;                       // key areas X (the result) and Y, shaped like incl
    unsigned* xj;
    real_t* ys;
    unsigned* yj;
    unsigned* cnt;                    // [chunk users] real keys of the row
};

__host__ __device__ constexpr size_t oi_ka(size_t k) { return (k + 3) & ~(size_t)3; }
// one-wave kernel: per wave a gather tile and the user's row
__host__ __device__ constexpr size_t oi_wave_lds(size_t k) { return (64 * (size_t)TI_SLOT + oi_ka(k) * TI_R + 15) & ~(size_t)15; }
// workgroup kernel: four gather tiles, the user's row, the key array and the count
__host__ __device__ constexpr size_t oi_run_lds(size_t k)
{
    return OI_WAVES * 64 * (size_t)TI_SLOT + ((oi_ka(k) * TI_R + 15) & ~(size_t)15) + OI_RUN * (TI_R + sizeof(unsigned)) + 16;
}
// LDS of a CU: 160 KB.  One-wave kernel: 68.8 KB (fp32) / 69.6 KB (fp64) per workgroup at k = 50, two workgroups per CU at every k.
// Workgroup kernel: 84.2 KB / 92.4 KB at k = 50, one workgroup per CU -- two would need the four gather tiles (68 KB) and the keys
// (16 / 24 KB) in 80 KB.
static_assert(2 * OI_WAVES * oi_wave_lds(TB_K_MAX) <= 160 * 1024, "two workgroups of order_wave_kernel per CU");
static_assert(oi_run_lds(TB_K_MAX) <= 160 * 1024 && 2 * oi_run_lds(50) > 160 * 1024, "one workgroup of order_run_kernel per CU");

// the user's row into LDS, zero padded to a multiple of four columns
__device__ __forceinline__ void oi_load_row(real_t* As, const real_t* Au, int k, unsigned t, unsigned nt)
{
    const int ka = (int)oi_ka((size_t)k);
    for (int c = (int)t; c < ka; c += (int)nt) As[c] = c < k ? Au[c] : (real_t)0;
}

__global__ __launch_bounds__(64 * OI_WAVES) void order_wave_kernel(OiArgs a)
{
    extern __shared__ __align__(16) unsigned char oi_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned item = blockIdx.x * OI_WAVES + wave;
    if (item >= a.n_items) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.k;
    unsigned char* Bs = oi_smem + wave * oi_wave_lds((size_t)k);   // [64][TI_SLOT]: the pass's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                     // [ka] the user's row, zero padded

    const OiItem it = a.items[item];
    const unsigned arow = a.users[it.ui];
    oi_load_row(As, a.A + (size_t)arow * (size_t)k, k, lane, 64);
    tb_wave_sync();

    const unsigned* lst = a.incl + it.p0;
    const unsigned npass = (it.len + 63) / 64;   // 1 .. OI_Q
    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };
    ti_u32x4 pre[TI_NI];
    real_t ks[OI_Q];
    unsigned kj[OI_Q];
#pragma unroll
    for (int q = 0; q < OI_Q; q++) { ks[q] = os_none_score(); kj[q] = TB_NONE; }

    unsigned j_cur = lane < it.len ? lst[lane] : TB_NONE;
    g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);
    for (unsigned pass = 0; pass < npass; pass++) {
        const unsigned nx = (pass + 1) * 64 + lane;
        const unsigned j_nxt = nx < it.len ? lst[nx] : TB_NONE;
        const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, pass, npass);
        const bool real = j_cur != TB_NONE && !tb_excluded(a.excl, it.ui, arow, j_cur);
#pragma unroll
        for (int q = 0; q < OI_Q; q++)
            if (pass == (unsigned)q) { ks[q] = real ? s : os_none_score(); kj[q] = real ? j_cur : TB_NONE; }
        j_cur = j_nxt;
    }

    os_wave_sort<OI_Q>(ks, kj, npass <= 1 ? 1u : npass == 2 ? 2u : (unsigned)OI_Q, lane);

    unsigned c = 0;
    real_t* o_score = ((it.flags & OI_AREA_Y) ? a.ys : a.xs) + it.p0;
    unsigned* o_ix = ((it.flags & OI_AREA_Y) ? a.yj : a.xj) + it.p0;
#pragma unroll
    for (int q = 0; q < OI_Q; q++) {
        c += (unsigned)__popcll(__ballot(kj[q] != TB_NONE));
        const unsigned e = 64u * q + lane;
        if (e < it.len) { o_score[e] = ks[q]; o_ix[e] = kj[q]; }
    }
    if (lane == 0) a.cnt[it.ui] = c;
}

// the sorted keys of a workgroup's row or run, from the key array in LDS to the item's area: p = OS_WG x E entries
template <int E> __device__ __forceinline__ void oi_sort_out(real_t* ss, unsigned* sj, unsigned t, unsigned len, real_t* o_score, unsigned* o_ix)
{
    real_t ks[E];
    unsigned kj[E];
#pragma unroll
    for (int r = 0; r < E; r++) { ks[r] = ss[OS_WG * r + t]; kj[r] = sj[OS_WG * r + t]; }
    os_wg_sort<E>(ks, kj, ss, sj, t);
#pragma unroll
    for (int r = 0; r < E; r++) {
        const unsigned e = OS_WG * r + t;
        if (e < len) { o_score[e] = ks[r]; o_ix[e] = kj[r]; }
    }
}

__global__ __launch_bounds__(64 * OI_WAVES) void order_run_kernel(OiArgs a)
{
    extern __shared__ __align__(16) unsigned char oi_smem[];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k = a.k;
    unsigned char* Bs = oi_smem + wave * 64 * TI_SLOT;                                 // this wave's gather tile
    real_t* As = (real_t*)(oi_smem + OI_WAVES * 64 * TI_SLOT);                         // [ka] the user's row, zero padded
    real_t* ss = (real_t*)((unsigned char*)As + ((oi_ka((size_t)k) * TI_R + 15) & ~(size_t)15));   // [OI_RUN] key scores
    unsigned* sj = (unsigned*)(ss + OI_RUN);                                           // [OI_RUN] key items
    unsigned* cnt = sj + OI_RUN;                                                       // real keys

    const OiItem it = a.items[blockIdx.x];   // (one workgroup per item: the grid is the item list)
    const unsigned arow = a.users[it.ui];
    oi_load_row(As, a.A + (size_t)arow * (size_t)k, k, t, OS_WG);
    if (t == 0) *cnt = 0;
    const unsigned p = it.len <= 512 ? 512u : it.len <= 1024 ? 1024u : (unsigned)OI_RUN;   // entries the network orders
    for (unsigned e = it.len + t; e < p; e += OS_WG) { ss[e] = os_none_score(); sj[e] = TB_NONE; }
    __syncthreads();

    // ---- gather and score: wave w owns passes w, w + OI_WAVES, ... ----
    const unsigned* lst = a.incl + it.p0;
    const unsigned npass = (it.len + 63) / 64;
    const unsigned mine = npass > wave ? (npass - wave + OI_WAVES - 1) / OI_WAVES : 0;
    const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };
    ti_u32x4 pre[TI_NI];
    unsigned pos = wave * 64 + lane;
    unsigned j_cur = pos < it.len ? lst[pos] : TB_NONE;
    unsigned real_keys = 0;
    if (mine) g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);
    for (unsigned lp = 0; lp < mine; lp++) {
        const unsigned nx = pos + 64 * OI_WAVES;
        const unsigned j_nxt = nx < it.len ? lst[nx] : TB_NONE;
        const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, lp, mine);
        const bool real = j_cur != TB_NONE && !tb_excluded(a.excl, it.ui, arow, j_cur);
        if (pos < it.len) { ss[pos] = real ? s : os_none_score(); sj[pos] = real ? j_cur : TB_NONE; }
        real_keys += (unsigned)__popcll(__ballot(real));
        j_cur = j_nxt;
        pos = nx;
    }
    if (lane == 0 && real_keys) atomicAdd(cnt, real_keys);   // (LDS, integer)
    __syncthreads();

    // ---- order and write ----
    real_t* o_score = ((it.flags & OI_AREA_Y) ? a.ys : a.xs) + it.p0;
    unsigned* o_ix = ((it.flags & OI_AREA_Y) ? a.yj : a.xj) + it.p0;
    if (t == 0) {
        if (it.flags & OI_PART) atomicAdd(a.cnt + it.ui, *cnt);   // (integer: the sum of a row's runs does not depend on their order)
        else a.cnt[it.ui] = *cnt;
    }
    if (p == 512) oi_sort_out<2>(ss, sj, t, it.len, o_score, o_ix);
    else if (p == 1024) oi_sort_out<4>(ss, sj, t, it.len, o_score, o_ix);
    else oi_sort_out<OI_E>(ss, sj, t, it.len, o_score, o_ix);
}

// One pass of the merge: runs of `width` entries of a row, pairwise, from the item's source area to the other.  The last run of a row
// may be shorter and may have no partner (the block is then a copy).
__global__ __launch_bounds__(OS_WG) void order_merge_kernel(const OmItem* items, unsigned width, real_t* xs, unsigned* xj, real_t* ys, unsigned* yj)
{
    __shared__ real_t ms[OS_MERGE_BLOCK];   // the piece of a, then the piece of b
    __shared__ unsigned mj[OS_MERGE_BLOCK];
    __shared__ real_t os[OS_MERGE_BLOCK];   // the block in order
    __shared__ unsigned oj[OS_MERGE_BLOCK];
    __shared__ unsigned cut[2];
    const unsigned t = threadIdx.x;
    const OmItem it = items[blockIdx.x];
    const real_t* src_s = (it.src ? ys : xs) + it.p0;
    const unsigned* src_j = (it.src ? yj : xj) + it.p0;
    real_t* dst_s = (it.src ? xs : ys) + it.p0;
    unsigned* dst_j = (it.src ? xj : yj) + it.p0;

    const unsigned at = it.block * OS_MERGE_BLOCK;          // the block's first entry of the row; OS_MERGE_BLOCK divides 2 width
    const unsigned ps = at / (2 * width) * (2 * width);     // where its pair of runs starts
    const unsigned la = min(width, it.len - ps), lb = min(width, it.len - ps - la);
    const real_t* as = src_s + ps;
    const unsigned* aj = src_j + ps;
    const real_t* bs = as + la;
    const unsigned* bj = aj + la;
    const unsigned o0 = at - ps, o1 = min(o0 + OS_MERGE_BLOCK, la + lb);
    if (t < 2) cut[t] = os_merge_path(as, aj, la, bs, bj, lb, t ? o1 : o0);
    __syncthreads();
    const unsigned i0 = cut[0], na = cut[1] - i0, n = o1 - o0, nb = n - na, b0 = o0 - i0;
    for (unsigned x = t; x < n; x += OS_WG) {
        const unsigned from = x < na ? i0 + x : la + b0 + (x - na);   // (b follows a in the source)
        ms[x] = as[from];
        mj[x] = aj[from];
    }
    __syncthreads();
    for (unsigned x = t; x < n; x += OS_WG) {
        const real_t s = ms[x];
        const unsigned j = mj[x];
        // a's entry x: behind the x before it and the entries of b that come before it; b's entry y: behind y and the entries of a
        // that come before it or equal it
        const unsigned place = x < na ? x + os_before(ms + na, mj + na, nb, s, j, false) : (x - na) + os_before(ms, mj, na, s, j, true);
        os[place] = s;
        oj[place] = j;
    }
    __syncthreads();
    for (unsigned x = t; x < n; x += OS_WG) {
        dst_s[ps + o0 + x] = os[x];
        dst_j[ps + o0 + x] = oj[x];
    }
}

inline unsigned oi_passes(size_t len)   // merge passes of a row: ceil(log2(runs))
{
    unsigned np = 0;
    for (size_t runs = pmf_ceil_div(len, OI_RUN); ((size_t)1 << np) < runs;) np++;
    return np;
}
constexpr unsigned OI_PASSES_MAX = 5;
static_assert(((size_t)OI_RUN << OI_PASSES_MAX) >= OI_MAX_ROW, "the longest row is merged in OI_PASSES_MAX passes");

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct OiLayout {
    size_t chunk_users;      // users per chunk
    size_t cell_cap;         // include indices (and keys per area) a chunk may carry
    size_t excl_cap;         // exclusion indices a chunk may carry
    size_t item_cap;         // work items of the two sorting kernels
    size_t mitem_cap;        // work items of all merge passes
    size_t users, ex_indptr, ex_indices, incl, items, mitems, cnt, xs, xj, ys, yj, total;
    OiLayout(size_t n_users, size_t n_cells, size_t dimB)
    {
        const size_t R = sizeof(real_t);
        n_users = std::max<size_t>(n_users, 1);
        dimB = std::max<size_t>(dimB, 1);
        chunk_users = std::min(n_users, TB_CHUNK_USERS_MAX);
        excl_cap = std::min(TB_BUDGET / 2 / sizeof(unsigned), chunk_users * dimB);   // section 1f's: half of the budget  (no overflow: 2^18 x 2^31)
        // per user: its row of A, exclusion row pointer, count and one work item; per cell: its index and a key in either area; a row
        // above R has at most len / R + 1 runs and, in each of OI_PASSES_MAX passes, len / OS_MERGE_BLOCK + 1 blocks -- rows above R number
        // at most cells / R
        const size_t per_user = 3 * sizeof(unsigned) + sizeof(OiItem);
        const size_t rest = TB_BUDGET - excl_cap * sizeof(unsigned) - chunk_users * per_user - 1024;   // (1024: alignment of the eleven parts, two spare entries)
        auto items_of = [](size_t cells) { return cells / OI_RUN + 1; };
        auto mitems_of = [](size_t cells) { return OI_PASSES_MAX * (cells / OS_MERGE_BLOCK + cells / OI_RUN + 1); };
        cell_cap = std::max<size_t>(n_cells, 1);
        auto bytes_of = [&](size_t cells) {
            return cells * (sizeof(unsigned) + 2 * (R + sizeof(unsigned))) + items_of(cells) * sizeof(OiItem) + mitems_of(cells) * sizeof(OmItem);
        };
        if (bytes_of(cell_cap) > rest) {
            cell_cap = rest / (sizeof(unsigned) + 2 * (R + sizeof(unsigned)) + 1);   // (the work items of a cell: under a byte)
            while (bytes_of(cell_cap) > rest) cell_cap -= OI_RUN;
        }
        item_cap = chunk_users + items_of(cell_cap);
        mitem_cap = mitems_of(cell_cap);
        TbTake take;
        users = take(chunk_users * sizeof(unsigned));
        ex_indptr = take((chunk_users + 1) * sizeof(unsigned));
        ex_indices = take(excl_cap * sizeof(unsigned));
        incl = take(cell_cap * sizeof(unsigned));
        items = take(item_cap * sizeof(OiItem));
        mitems = take(mitem_cap * sizeof(OmItem));
        cnt = take(chunk_users * sizeof(unsigned));
        xs = take(cell_cap * R);
        xj = take(cell_cap * sizeof(unsigned));
        ys = take(cell_cap * R);
        yj = take(cell_cap * sizeof(unsigned));
        total = take.o;
    }
};
static_assert(TB_BUDGET / 2 - TB_CHUNK_USERS_MAX * 28 - 1024 >= OI_MAX_ROW * 64, "the smallest chunk holds the longest row many times over");

}  // namespace

extern "C" size_t poismf_hip_order_include_scratch_bytes(size_t n_users, size_t n_cells, size_t dimB, size_t k)
{
    (void)k;   // (the factors' chunks live in LDS: no part of the scratch depends on k)
    return OiLayout(n_users, n_cells, dimB).total;
}
extern "C" size_t poismf_hip_order_include_run(void) { return OI_RUN; }
extern "C" size_t poismf_hip_order_include_wave_row(void) { return OI_WAVE_ROW; }

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_order_include_check(const sparse_ix* users, size_t n_users, size_t dimA, size_t dimB, size_t k, const sparse_ix* incl_indptr,
                                   const sparse_ix* incl_indices, const sparse_ix* excl_indptr, const sparse_ix* excl_indices)
{
    if (k < 1 || k > TB_K_MAX || dimB > 0x7fffffffull || dimA > 0x7fffffffull) return 2;
    if (users == nullptr || incl_indptr == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++)
        if ((size_t)users[i] >= dimA) return 2;
    if (!tb_rows_ok(incl_indptr, incl_indices, n_users, dimB, OI_MAX_ROW)) return 2;
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    return 0;
}

// ---- core on device-resident factors (tb_batch.hpp) ----
int poismf_hip_order_include_core(hipStream_t stream, const real_t* dA, const real_t* dB, size_t dimB, size_t k, bool compact_A,
                                  const sparse_ix* users, size_t n_users, const sparse_ix* incl_indptr, const sparse_ix* incl_indices,
                                  PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, void** d_scratch,
                                  size_t* scratch_cap, sparse_ix* out_ix, real_t* out_score, sparse_ix* out_count)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const size_t cell0 = (size_t)incl_indptr[0];
    const OiLayout L(n_users, (size_t)incl_indptr[n_users] - cell0, dimB);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(order_wave_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(OI_WAVES * oi_wave_lds(TB_K_MAX))));
    TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(order_run_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)oi_run_lds(TB_K_MAX)));

    OiArgs a;
    a.A = dA;
    a.B = dB;
    a.users = (const unsigned*)(base + L.users);
    a.incl = (const unsigned*)(base + L.incl);
    a.k = (int)k;
    a.xs = (real_t*)(base + L.xs);
    a.xj = (unsigned*)(base + L.xj);
    a.ys = (real_t*)(base + L.ys);
    a.yj = (unsigned*)(base + L.yj);
    a.cnt = (unsigned*)(base + L.cnt);
    std::vector<unsigned> hu, hp, hx, hi, hc;
    std::vector<OiItem> short_items, run_items;
    std::vector<OmItem> merge_items[OI_PASSES_MAX];
    auto row_len = [&](size_t i) { return (size_t)incl_indptr[i + 1] - (size_t)incl_indptr[i]; };
    for (size_t u0 = 0; u0 < n_users;) {
        // the chunk: up to chunk_users users whose include lists fit the cell areas together; the exclusion lists may cut it shorter
        size_t fit = 0;
        for (size_t ni = 0; u0 + fit < n_users && fit < L.chunk_users; fit++) {
            if (fit > 0 && ni + row_len(u0 + fit) > L.cell_cap) break;
            ni += row_len(u0 + fit);
        }
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, fit, L.excl_cap, excl_indptr, excl_indices, users, compact_A, seen, tb_chunk_dev(base, L), hu, hp, hx,
                           stream))
            return 1;
        const size_t nu = u1 - u0, i_base = (size_t)incl_indptr[u0], ni = (size_t)incl_indptr[u1] - i_base;
        // the plan: a work item per row or run, and per merge pass one per block of every row still being merged
        short_items.clear();
        run_items.clear();
        for (auto& m : merge_items) m.clear();
        for (size_t i = 0; i < nu; i++) {
            const size_t len = row_len(u0 + i), p0 = (size_t)incl_indptr[u0 + i] - i_base;
            if (len == 0) continue;   // (its count stays 0)
            if (len <= OI_WAVE_ROW) {
                short_items.push_back({ (unsigned)i, (unsigned)p0, (unsigned)len, 0u });
            } else if (len <= OI_RUN) {
                run_items.push_back({ (unsigned)i, (unsigned)p0, (unsigned)len, 0u });
            } else {
                const unsigned np = oi_passes(len);   // the runs start in Y when the passes are odd in number: the last one writes X
                for (size_t r0 = 0; r0 < len; r0 += OI_RUN)
                    run_items.push_back({ (unsigned)i, (unsigned)(p0 + r0), (unsigned)std::min(OI_RUN, len - r0), OI_PART | ((np & 1u) ? OI_AREA_Y : 0u) });
                for (unsigned m = 0; m < np; m++)
                    for (size_t b = 0; b * OS_MERGE_BLOCK < len; b++) merge_items[m].push_back({ (unsigned)p0, (unsigned)len, (unsigned)b, (np + m) & 1u });
            }
        }
        // one upload each: the rows' items then the runs', and every pass's blocks one pass after the other
        const size_t n_short = short_items.size();
        short_items.insert(short_items.end(), run_items.begin(), run_items.end());
        size_t n_pass[OI_PASSES_MAX], n_merge = 0;
        for (unsigned m = 0; m < OI_PASSES_MAX; m++) n_merge += n_pass[m] = merge_items[m].size();
        for (unsigned m = 1; m < OI_PASSES_MAX; m++) merge_items[0].insert(merge_items[0].end(), merge_items[m].begin(), merge_items[m].end());
        if (short_items.size() > L.item_cap || n_merge > L.mitem_cap || ni > L.cell_cap) return 1;   // (cannot happen: OiLayout sizes the areas for any chunk)
        hi.resize(ni);
        for (size_t p = 0; p < ni; p++) hi[p] = (unsigned)incl_indices[i_base + p];
        hc.assign(nu, 0u);
        TB_TRY(pmf_upload(base + L.incl, hi.data(), ni * sizeof(unsigned), stream));
        TB_TRY(pmf_upload(base + L.items, short_items.data(), short_items.size() * sizeof(OiItem), stream));
        TB_TRY(pmf_upload(base + L.mitems, merge_items[0].data(), n_merge * sizeof(OmItem), stream));
        TB_TRY(pmf_upload(base + L.cnt, hc.data(), nu * sizeof(unsigned), stream));
        if (n_short) {
            a.items = (const OiItem*)(base + L.items);
            a.n_items = (unsigned)n_short;
            hipLaunchKernelGGL(order_wave_kernel, dim3((unsigned)pmf_ceil_div(n_short, OI_WAVES)), dim3(64 * OI_WAVES), OI_WAVES * oi_wave_lds(k), stream, a);
            TB_TRY(hipGetLastError());
        }
        if (!run_items.empty()) {
            a.items = (const OiItem*)(base + L.items) + n_short;
            a.n_items = (unsigned)run_items.size();
            hipLaunchKernelGGL(order_run_kernel, dim3((unsigned)run_items.size()), dim3(64 * OI_WAVES), oi_run_lds(k), stream, a);
            TB_TRY(hipGetLastError());
        }
        for (size_t m = 0, m_at = 0; m < OI_PASSES_MAX && n_pass[m]; m_at += n_pass[m], m++) {
            hipLaunchKernelGGL(order_merge_kernel, dim3((unsigned)n_pass[m]), dim3(OS_WG), 0, stream, (const OmItem*)(base + L.mitems) + m_at,
                               (unsigned)(OI_RUN << m), a.xs, a.xj, a.ys, a.yj);
            TB_TRY(hipGetLastError());
        }
        // the chunk's results: area X, shaped like the lists
        TB_TRY(pmf_download(hi.data(), a.xj, ni * sizeof(unsigned), stream));
        const size_t o0 = i_base - cell0;
        for (size_t p = 0; p < ni; p++) out_ix[o0 + p] = hi[p] == TB_NONE ? POISMF_HIP_TOPN_NONE : (sparse_ix)hi[p];
        if (out_score != nullptr) TB_TRY(pmf_download(out_score + o0, a.xs, ni * sizeof(real_t), stream));
        if (out_count != nullptr) {
            TB_TRY(pmf_download(hc.data(), a.cnt, nu * sizeof(unsigned), stream));
            for (size_t i = 0; i < nu; i++) out_count[u0 + i] = (sparse_ix)hc[i];
        }
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_order_include(const real_t* A, const real_t* B, int k, size_t dimA, size_t dimB, const sparse_ix* users, size_t n_users,
                             const sparse_ix* incl_indptr, const sparse_ix* incl_indices, const sparse_ix* excl_indptr,
                             const sparse_ix* excl_indices, sparse_ix* out_ix, real_t* out_score, sparse_ix* out_count)
{
    if (n_users == 0) return 0;
    if (k < 1 || A == nullptr || B == nullptr || out_ix == nullptr) return 2;
    if (const int rc = poismf_hip_order_include_check(users, n_users, dimA, dimB, (size_t)k, incl_indptr, incl_indices, excl_indptr, excl_indices))
        return rc;
    return tb_dropin(A, B, (size_t)k, dimA, dimB, users, n_users,
                     [&](hipStream_t st, const real_t* dA, const real_t* dB, bool compact, void** d_scratch, size_t* scratch_cap) {
                         return poismf_hip_order_include_core(st, dA, dB, dimB, (size_t)k, compact, users, n_users, incl_indptr, incl_indices, nullptr,
                                                              excl_indptr, excl_indices, d_scratch, scratch_cap, out_ix, out_score, out_count);
                     });
}

}  // extern "C"
