// list_eval.hip -- list-wise evaluation of given top-N lists (include/poismf_hip.h, section 1q): per row of `lists` the positions of the
// row's held-out items, the fixed-point sum of the pairwise cosines of its items, its length, and per item how many rows list it.
//
// ONE WAVE owns one row, four such waves share a workgroup and nothing else -- no workgroup barrier, every LDS region belongs to one
// wave (the shape of topn_diverse_mmr_kernel, topn_diverse.hip).  The row of `lists` lies in the wave's LDS; lane l owns positions l and
// l + 64.  Per wave:
//   positions  the lanes stride over the row's held-out cells, each scans the list in LDS: at most 128 compares per cell;
//   exposure   one unsigned atomic add in global memory per real entry -- the only atomics, integer, so the counts are exact;
//   cosines    for q = 1 .. c - 1 the row B[j_q] goes to LDS and is read back at a wave-uniform address; the rows at the positions
//              below q go through tb_gather.hpp's TiGather 64 at a time (one pass, two from q = 65 on) and ti_pass multiplies them,
//              k-ordered, against B[j_q]; the first chunk of the next pass travels in registers.  Then section 1q's two rounded
//              multiplications (le_mul: section 1p's tv_mul), the quantisation to units of 2^-40 and an int64 sum per lane; one DPP
//              reduction of the sums at the end.  Integer sums: the answer does not depend on which lane added what.
// The rows are gathered again, out of the caches, for every q: c (c - 1) / 2 chains per row, one code path for every k and n_list.
//
// The host side: norms and exposure counts go in front of the chunk's parts (LeLayout); the chunk loop cuts the users by count and by
// held-out cells, so that the one scratch allocation stays inside the budget whatever n_users and the number of cells.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/poismf_hip.h"
#include "cores.hpp"
#include "devmem.hpp"
#include "wave_ops.hpp"
#include "tb_tile.hpp"
#include "tb_gather.hpp"
#include "tb_batch.hpp"

namespace {

constexpr int LE_WAVES = 4;                               // rows per workgroup
constexpr unsigned LE_N_MAX = (unsigned)TB_N_TOP_MAX;     // positions of a row: two per lane
constexpr size_t LE_MAX_ITEMS = POISMF_HIP_LIST_EVAL_MAX_ITEMS;
constexpr size_t LE_BUDGET = (size_t)POISMF_HIP_LIST_EVAL_BUDGET_MB << 20;
constexpr size_t LE_ROW_MAX = POISMF_HIP_RANK_BATCH_MAX_ROW;
constexpr size_t LE_SLACK = 256;                          // what TbTake's alignment of the eight parts can add
constexpr size_t LE_LDS_LIMIT = 96 * 1024;
static_assert(LE_N_MAX == 128, "lane l owns positions l and l + 64");
static_assert(LE_MAX_ITEMS * (sizeof(double) + sizeof(unsigned)) + LE_SLACK + 4 + (4 * LE_N_MAX + 16) + LE_ROW_MAX * 8 <= LE_BUDGET,
              "the budget: norms in double and counts at the item limit, and one user with the longest held-out row behind them");

struct LeArgs {
    const real_t* B;                  // [dimB x k]
    const real_t* inv;                // [dimB] item_inv_norm, or nullptr: no cosines
    int k;
    unsigned n_users, n_list;
    const unsigned* lists;            // [n_users][n_list]: real entries first, then TB_NONE
    const unsigned* cell_ptr;         // [n_users + 1] the rows' first cells, or nullptr: no held-out cells
    const unsigned* cell_item;        // [cells]
    unsigned* out_pos;                // [cells]
    long long* out_cos;               // [n_users]
    unsigned* out_len;                // [n_users]
    unsigned* exposure;               // [dimB], zeroed before the first chunk
};

// Section 1q's multiplication, rounded once (topn_diverse.hip's tv_mul): the product goes through an empty asm statement, which no
// contraction can see through and which emits nothing.
__device__ __forceinline__ float le_keep(float x) { __asm__ volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ double le_keep(double x) { __asm__ volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float le_mul(float a, float b) { return le_keep(__fmul_rn(a, b)); }
__device__ __forceinline__ double le_mul(double a, double b) { return le_keep(__dmul_rn(a, b)); }

// Q of section 1q: NaN counts as 0, clamped to [-2, 2], units of 2^-40 (the product is exact), round half to even
__device__ __forceinline__ long long le_quant(real_t cs)
{
    double t = (double)cs;
    t = t != t ? 0.0 : t;
    t = t < -2.0 ? -2.0 : (t > 2.0 ? 2.0 : t);
    return __double2ll_rn(t * (double)(1ull << POISMF_HIP_LIST_COS_SHIFT));
}

template <int CTRL> __device__ __forceinline__ long long le_dpp(long long v)
{
    const unsigned lo = (unsigned)pmf::dpp_i32<CTRL>((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)pmf::dpp_i32<CTRL>((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long le_read_lane(long long v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// the wave's sum: four DPP steps inside each row of 16 lanes (wave_ops.hpp's wave_reduce), then the four rows
__device__ __forceinline__ long long le_wave_sum(long long x)
{
    x += le_dpp<0xB1>(x);
    x += le_dpp<0x4E>(x);
    x += le_dpp<0x141>(x);
    x += le_dpp<0x140>(x);
    return (le_read_lane(x, 0) + le_read_lane(x, 16)) + (le_read_lane(x, 32) + le_read_lane(x, 48));
}

// a wave's LDS: the gather's tile, the row B[j_q] (zero padded to four columns) and the row of `lists`
__host__ __device__ inline size_t le_wave_lds(size_t k)
{
    const size_t ka = (k + 3) & ~(size_t)3;
    return (64 * (size_t)TI_SLOT + ka * TI_R + LE_N_MAX * sizeof(unsigned) + 15) & ~(size_t)15;
}
static_assert(LE_WAVES * (64 * (size_t)TI_SLOT + TB_K_MAX * sizeof(real_t) + LE_N_MAX * sizeof(unsigned) + 16) <= LE_LDS_LIMIT,
              "four waves' tiles, rows and lists fit LDS at the largest k");

__global__ __launch_bounds__(64 * LE_WAVES) void list_eval_kernel(LeArgs a)
{
    extern __shared__ __align__(16) unsigned char le_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned u = blockIdx.x * LE_WAVES + wave;
    if (u >= a.n_users) return;   // (no workgroup barrier below: the waves of a workgroup share nothing)
    const int k = a.k;
    const int ka = (k + 3) & ~3;
    unsigned char* Bs = le_smem + wave * le_wave_lds((size_t)k);   // [64][TI_SLOT]: a pass's rows of B, one chunk of columns
    real_t* As = (real_t*)(Bs + 64 * TI_SLOT);                      // [ka] the row of position q, zero padded
    unsigned* li = (unsigned*)(As + ka);                            // [LE_N_MAX] the row of `lists`, TB_NONE behind n_list

    const unsigned* row = a.lists + (size_t)u * a.n_list;
    for (unsigned e = lane; e < LE_N_MAX; e += 64) li[e] = e < a.n_list ? row[e] : TB_NONE;
    tb_wave_sync();

    // c: the row's real entries, a prefix of it (the checks refuse a real entry behind an empty one)
    unsigned c = 0;
    for (unsigned p0 = 0; p0 < LE_N_MAX; p0 += 64) {
        const unsigned long long real = __ballot(li[p0 + lane] != TB_NONE);
        const unsigned lead = real == ~0ull ? 64u : (unsigned)__builtin_ctzll(~real);
        c += lead;
        if (lead < 64) break;
    }
    if (lane == 0) a.out_len[u] = c;
    for (unsigned e = lane; e < c; e += 64) atomicAdd(a.exposure + li[e], 1u);

    if (a.cell_ptr != nullptr) {
        const unsigned p1 = a.cell_ptr[u + 1];
        for (unsigned i = a.cell_ptr[u] + lane; i < p1; i += 64) {
            const unsigned item = a.cell_item[i];
            unsigned pos = POISMF_HIP_LIST_ABSENT;
            for (unsigned q = 0; q < c; q++)
                if (li[q] == item) pos = q;   // (the real entries are distinct)
            a.out_pos[i] = pos;
        }
    }

    if (a.inv == nullptr) return;
    long long acc = 0;
    if (c >= 2) {
        const real_t inv_lo = lane < c ? a.inv[li[lane]] : (real_t)0;
        const real_t inv_hi = 64 + lane < c ? a.inv[li[64 + lane]] : (real_t)0;
        const TiGather g = { (const char*)a.B, Bs, k, lane >> 2, lane & 3 };   // (tb_gather.hpp) this lane loads piece fq + 4 g of rows frow + 16 r
        ti_u32x4 pre[TI_NI];
        unsigned j_cur = lane < 1 ? li[0] : TB_NONE;                           // the rows of q = 1: position 0
        g.fetch(pre, j_cur, 0, k < TI_KC ? k : TI_KC);
        for (unsigned q = 1; q < c; q++) {
            const unsigned jq = pmf::uniform(li[q]);
            const real_t inv_q = a.inv[jq];
            tb_wave_sync();                    // the wave is done with the row of the step before
            for (int cc = (int)lane; cc < ka; cc += 64) As[cc] = cc < k ? a.B[(size_t)jq * (size_t)k + (size_t)cc] : (real_t)0;
            tb_wave_sync();
            const unsigned npass = (q + 63) / 64;   // the positions below q, 64 at a time
            for (unsigned p = 0; p < npass; p++) {
                // the rows that follow these: the next pass's, or the first pass of q + 1 (positions 0 .. q)
                const bool last = p + 1 == npass;
                const bool follow = !last || q + 1 < c;
                const unsigned nx = last ? lane : 64 * (p + 1) + lane;
                const unsigned below = last ? q + 1 : q;
                const unsigned j_nxt = follow && nx < below ? li[nx] : TB_NONE;
                const real_t s = ti_pass(g, pre, As, j_cur, j_nxt, 0u, follow ? 2u : 1u);
                if (j_cur != TB_NONE) acc += le_quant(le_mul(le_mul(s, inv_q), p == 0 ? inv_lo : inv_hi));
                j_cur = j_nxt;
            }
        }
    }
    acc = le_wave_sum(acc);
    if (lane == 0) a.out_cos[u] = acc;
}

// The one scratch allocation of a call, in bytes from the start: the inverse norms and the exposure counts, once per call, and a
// chunk of users -- their rows, first cells, cells (item and position), sums and lengths.  total == 0: the budget is below what the
// norms, the counts, one user and the longest held-out row the call can hold need.
struct LeLayout {
    size_t chunk_users, cell_cap;
    size_t inv, expo, lists, cell_ptr, cell_item, pos, cos, len, total;
    LeLayout(size_t n_users, size_t n_list, size_t n_cells, size_t dimB, size_t budget_bytes)
    {
        n_users = std::max<size_t>(n_users, 1);
        n_list = std::min(std::max<size_t>(n_list, 1), TB_N_TOP_MAX);
        dimB = std::min(std::max<size_t>(dimB, 1), LE_MAX_ITEMS);
        const size_t budget = budget_bytes == 0 || budget_bytes > LE_BUDGET ? LE_BUDGET : budget_bytes;
        const size_t fixed = pmf_round_up(dimB * sizeof(real_t), 32) + pmf_round_up(dimB * sizeof(unsigned), 32) + LE_SLACK + sizeof(unsigned);
        const size_t per_user = n_list * sizeof(unsigned) + sizeof(unsigned) + sizeof(long long) + sizeof(unsigned);
        const size_t row_cells = std::min(n_cells, LE_ROW_MAX);
        chunk_users = cell_cap = inv = expo = lists = cell_ptr = cell_item = pos = cos = len = total = 0;
        if (budget < fixed + per_user + row_cells * 8) return;
        const size_t room = budget - fixed;
        cell_cap = std::min(n_cells, std::max(row_cells, room / 2 / 8));
        chunk_users = std::min({ n_users, (room - cell_cap * 8) / per_user, TB_CHUNK_USERS_MAX });
        TbTake take;
        inv = take(dimB * sizeof(real_t));
        expo = take(dimB * sizeof(unsigned));
        lists = take(chunk_users * n_list * sizeof(unsigned));
        cell_ptr = take((chunk_users + 1) * sizeof(unsigned));
        cell_item = take(cell_cap * sizeof(unsigned));
        pos = take(cell_cap * sizeof(unsigned));
        cos = take(chunk_users * sizeof(long long));
        len = take(chunk_users * sizeof(unsigned));
        total = take.o;
    }
};

size_t le_cells(const sparse_ix* test_indptr, size_t n_users) { return test_indptr ? (size_t)test_indptr[n_users] - (size_t)test_indptr[0] : 0; }

}  // namespace

extern "C" size_t poismf_hip_list_eval_scratch_bytes(size_t n_users, size_t n_list, size_t n_cells, size_t dimB, size_t budget_bytes)
{
    return LeLayout(n_users, n_list, n_cells, dimB, budget_bytes).total;
}

// The argument checks of both entry points: 0, or 2.  No device call.
int poismf_hip_list_eval_check(const sparse_ix* lists, size_t n_users, size_t n_list, size_t dimB, size_t k, const real_t* item_inv_norm,
                               const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes, const unsigned int* out_pos,
                               const long long* out_cos, const unsigned int* out_len, const unsigned int* exposure)
{
    if (lists == nullptr || out_len == nullptr || exposure == nullptr) return 2;
    if (n_list == 0 || n_list > TB_N_TOP_MAX || k < 1 || k > TB_K_MAX || dimB > LE_MAX_ITEMS) return 2;
    if (item_inv_norm != nullptr && out_cos == nullptr) return 2;
    // a repeated entry: the row's items go into an open-addressed table of twice the longest row, whose slots carry the row they were
    // written for, so nothing is cleared between rows and nothing is sorted
    constexpr size_t SLOTS = 2 * TB_N_TOP_MAX;
    static_assert((SLOTS & (SLOTS - 1)) == 0 && SLOTS == 256, "the slot is the top eight bits of the hash");
    size_t key[SLOTS], owner[SLOTS] = {};
    for (size_t u = 0; u < n_users; u++) {
        const sparse_ix* l = lists + u * n_list;
        size_t c = 0;
        for (size_t e = 0; e < n_list; e++) {
            if (l[e] == POISMF_HIP_TOPN_NONE) continue;
            if (c != e || (long long)l[e] < 0 || (size_t)l[e] >= dimB) return 2;   // (c != e: an empty entry lies in front of this one)
            c++;
            const size_t j = (size_t)l[e];
            size_t h = (size_t)(((unsigned long long)j * 0x9E3779B97F4A7C15ull) >> 56);
            for (; owner[h] == u + 1; h = (h + 1) & (SLOTS - 1))
                if (key[h] == j) return 2;
            owner[h] = u + 1;
            key[h] = j;
        }
    }
    if (test_indptr != nullptr) {
        if (!tb_rows_ok(test_indptr, test_indices, n_users, dimB, LE_ROW_MAX)) return 2;
        if (le_cells(test_indptr, n_users) > 0 && out_pos == nullptr) return 2;
    }
    for (size_t j = 0; item_inv_norm != nullptr && j < dimB; j++)
        if (!std::isfinite(item_inv_norm[j]) || item_inv_norm[j] < (real_t)0) return 2;   // (-0 is 0)
    if (LeLayout(n_users, n_list, le_cells(test_indptr, n_users), dimB, budget_bytes).total == 0) return 2;
    return 0;
}

// ---- core on a device-resident B (cores.hpp) ----
int poismf_hip_list_eval_run(hipStream_t stream, const real_t* dB, size_t dimB, size_t k, const sparse_ix* lists, size_t n_users, size_t n_list,
                             const real_t* item_inv_norm, const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes,
                             void** d_scratch, size_t* scratch_cap, unsigned int* out_pos, long long* out_cos, unsigned int* out_len,
                             unsigned int* exposure)
{
    const LeLayout L(n_users, n_list, le_cells(test_indptr, n_users), dimB, budget_bytes);
    if (L.total == 0) return 1;   // (cannot happen: the checks refuse such a budget)
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    const size_t lds = LE_WAVES * le_wave_lds(k);
    if (lds > LE_LDS_LIMIT) return 1;   // (cannot happen: the static_assert above covers the largest k)
    {   // the kernel's LDS limit is raised once per device and process (a bit per device; a device beyond the mask asks every time)
        static std::atomic<unsigned long long> raised{ 0 };
        int device = 0;
        TB_TRY(hipGetDevice(&device));
        const unsigned long long bit = device >= 0 && device < 64 ? 1ull << device : 0;
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            TB_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(list_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LE_LDS_LIMIT));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }

    if (item_inv_norm != nullptr) TB_TRY(pmf_upload(base + L.inv, item_inv_norm, dimB * sizeof(real_t), stream));
    TB_TRY(hipMemsetAsync(base + L.expo, 0, dimB * sizeof(unsigned), stream));

    LeArgs a;
    a.B = dB;
    a.inv = item_inv_norm != nullptr ? (const real_t*)(base + L.inv) : nullptr;
    a.k = (int)k;
    a.n_list = (unsigned)n_list;
    a.lists = (const unsigned*)(base + L.lists);
    a.cell_ptr = test_indptr != nullptr ? (const unsigned*)(base + L.cell_ptr) : nullptr;
    a.cell_item = (const unsigned*)(base + L.cell_item);
    a.out_pos = (unsigned*)(base + L.pos);
    a.out_cos = (long long*)(base + L.cos);
    a.out_len = (unsigned*)(base + L.len);
    a.exposure = (unsigned*)(base + L.expo);

    std::vector<unsigned> hl, hp, hx;
    try {
        for (size_t u0 = 0; u0 < n_users;) {
            // the chunk: up to chunk_users users whose held-out rows fit cell_cap cells together
            size_t u1 = u0, nc = 0;
            while (u1 < n_users && u1 - u0 < L.chunk_users) {
                const size_t len = test_indptr ? (size_t)test_indptr[u1 + 1] - (size_t)test_indptr[u1] : 0;
                if (nc + len > L.cell_cap) break;
                nc += len;
                u1++;
            }
            if (u1 == u0) return 1;   // (cannot happen: cell_cap holds the longest row)
            const size_t nu = u1 - u0;
            hl.resize(nu * n_list);
            for (size_t i = 0; i < nu * n_list; i++) {
                const sparse_ix j = lists[u0 * n_list + i];
                hl[i] = j == POISMF_HIP_TOPN_NONE ? TB_NONE : (unsigned)j;
            }
            TB_TRY(pmf_upload(base + L.lists, hl.data(), nu * n_list * sizeof(unsigned), stream));
            const size_t p_base = test_indptr ? (size_t)test_indptr[u0] : 0;
            if (test_indptr != nullptr) {
                hp.resize(nu + 1);
                hx.resize(nc);
                for (size_t i = 0; i <= nu; i++) hp[i] = (unsigned)((size_t)test_indptr[u0 + i] - p_base);
                for (size_t p = 0; p < nc; p++) hx[p] = (unsigned)test_indices[p_base + p];
                TB_TRY(pmf_upload(base + L.cell_ptr, hp.data(), (nu + 1) * sizeof(unsigned), stream));
                TB_TRY(pmf_upload(base + L.cell_item, hx.data(), nc * sizeof(unsigned), stream));
            }
            a.n_users = (unsigned)nu;
            hipLaunchKernelGGL(list_eval_kernel, dim3((unsigned)pmf_ceil_div(nu, LE_WAVES)), dim3(64 * LE_WAVES), lds, stream, a);
            TB_TRY(hipGetLastError());
            if (test_indptr != nullptr) TB_TRY(pmf_download(out_pos + (p_base - (size_t)test_indptr[0]), a.out_pos, nc * sizeof(unsigned), stream));
            if (item_inv_norm != nullptr) TB_TRY(pmf_download(out_cos + u0, a.out_cos, nu * sizeof(long long), stream));
            TB_TRY(pmf_download(out_len + u0, a.out_len, nu * sizeof(unsigned), stream));
            u0 = u1;
        }
    } catch (const std::bad_alloc&) {
        return 1;
    }
    TB_TRY(pmf_download(exposure, a.exposure, dimB * sizeof(unsigned), stream));
    return 0;
}

extern "C" {

int poismf_hip_list_eval(const real_t* B, int k, size_t dimB, const sparse_ix* lists, size_t n_users, size_t n_list, const real_t* item_inv_norm,
                         const sparse_ix* test_indptr, const sparse_ix* test_indices, size_t budget_bytes, unsigned int* out_pos,
                         long long* out_cos, unsigned int* out_len, unsigned int* exposure)
{
    if (n_users == 0) return 0;
    if (k < 1 || B == nullptr) return 2;
    if (const int rc = poismf_hip_list_eval_check(lists, n_users, n_list, dimB, (size_t)k, item_inv_norm, test_indptr, test_indices, budget_bytes,
                                                  out_pos, out_cos, out_len, exposure))
        return rc;
    // B goes to the device of POISMF_HIP_DEVICE, and everything is freed again
    const int device = pmf_env_device();
    if (hipSetDevice(device) != hipSuccess) return 1;
    const hipStream_t st = nullptr;
    real_t* dB = nullptr;
    void* d_scratch = nullptr;
    size_t scratch_cap = 0;
    int rc = 1;
    if (pmf_alloc(&dB, dimB * (size_t)k * sizeof(real_t) + 16, st) == hipSuccess &&
        pmf_upload_big(dB, B, dimB * (size_t)k * sizeof(real_t), device, st) == hipSuccess)
        rc = poismf_hip_list_eval_run(st, dB, dimB, (size_t)k, lists, n_users, n_list, item_inv_norm, test_indptr, test_indices, budget_bytes,
                                      &d_scratch, &scratch_cap, out_pos, out_cos, out_len, exposure);
    pmf_free(dB, st);
    pmf_free(d_scratch, st);
    return rc;
}

}  // extern "C"
