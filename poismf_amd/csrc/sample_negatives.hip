// sample_negatives.hip -- negative sampling on the device (include/poismf_hip.h, section 1t): for many users at once, m distinct items
// per user that are not in the user's exclusion set, drawn uniformly or by integer item weights from a counter-based stream
// (Philox4x32-10, philox.hpp) that belongs to the user's id -- the candidate lists the sampled evaluation (sections 1h, 1j, 1s) ranks
// among.  A row is a function of (seed, u, m, dimB, E(u), weights): the header's sequential rule "walk the draws upward, accept what
// is admissible and not accepted before, stop at m accepts or at the cap" is carried out 64 draws at a time.
//
// One wave per user.  The draw itself -- the Philox block, the candidate, the open-addressing table in LDS in which the earliest draw of
// equal items wins, the ballot cut -- is sn_draw_row (sn_draw.hpp), which the fused sampled ranks (rank_sampled.hip) call too; the
// admissibility test here is tb_excluded: the chunk's staged list and the resident row.  What this kernel adds is
//   the row   a u32 bitonic network over the list in LDS (padded with TB_NONE to a power of two, which is also the row's padding).
// No float anywhere.
//
// Two instances by LDS: m <= SN_SMALL_M four waves per workgroup, one user each, 3 KB per wave; above, one wave per workgroup with
// the table sized to m -- 48 KB at m = 4096, 56 KB with the coarse index, two workgroups per CU and more for a smaller m.
//
// The host side cuts the batch into chunks of users so that ONE scratch allocation of at most POISMF_HIP_TOPN_BATCH_BUDGET_MB holds
// the prefix sums, a chunk's users, stream ids, exclusion lists and rows (SnLayout; poismf_hip_sample_negatives_scratch_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/poismf_hip.h"
#include "devmem.hpp"
#include "tb_tile.hpp"
#include "tb_batch.hpp"
#include "sn_draw.hpp"

namespace {

static_assert(SN_MAX_M * 4 + 2 * SN_MAX_M * 4 + SN_COARSE * 8 <= 80 * 1024, "two workgroups of the largest row per CU");

struct SnArgs {
    const unsigned* users;                // the chunk's rows of A (exclude_seen)
    const unsigned long long* streams;    // the chunk's stream ids
    unsigned n_users;
    unsigned list_cap;                    // list entries (a power of two >= m) per wave
    SnDraw d;                             // m, the cap, the key, the table's size, the weights' prefix sums
    TbExcl excl;                          // E(u) of the chunk's users
    unsigned* items;                      // [chunk users x m]
    unsigned* cnt;                        // [chunk users]
    unsigned* draws;                      // [chunk users]
};

// ascending bitonic network of one wave over lst[0 .. p), p a power of two
__device__ __forceinline__ void sn_wave_sort(unsigned* lst, unsigned p, unsigned lane)
{
    for (unsigned k2 = 2; k2 <= p; k2 <<= 1)
        for (unsigned dist = k2 >> 1; dist > 0; dist >>= 1) {
            for (unsigned t = lane; t < p / 2; t += 64) {
                const unsigned i = ((t & ~(dist - 1)) << 1) | (t & (dist - 1));   // the pair's lower entry: bit `dist` clear
                const unsigned x = lst[i], y = lst[i + dist];
                if ((x > y) == ((i & k2) == 0)) { lst[i] = y; lst[i + dist] = x; }
            }
            tb_wave_sync();
        }
}

template <int WAVES, bool WEIGHTED> __global__ __launch_bounds__(64 * WAVES) void sample_negatives_kernel(SnArgs a)
{
    extern __shared__ __align__(16) unsigned char sn_smem[];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* coarse = (const unsigned long long*)sn_smem;
    if (WEIGHTED) {
        unsigned long long* cs = (unsigned long long*)sn_smem;
        for (unsigned t = threadIdx.x; t < a.d.n_coarse; t += 64 * WAVES) cs[t] = a.d.coarse[t];
        __syncthreads();   // (the only workgroup barrier: from here on the waves share nothing else)
    }
    const unsigned ui = blockIdx.x * WAVES + wave;
    if (ui >= a.n_users) return;
    const unsigned slots = 1u << a.d.log_slots;
    unsigned* tab = (unsigned*)(sn_smem + (WEIGHTED ? SN_COARSE * sizeof(unsigned long long) : 0)) + (size_t)wave * (slots + a.list_cap);
    unsigned* lst = tab + slots;
    for (unsigned e = lane; e < a.list_cap; e += 64) lst[e] = TB_NONE;

    const unsigned arow = a.users[ui];
    const unsigned m = a.d.m;
    unsigned draws;
    const unsigned count = sn_draw_row<WEIGHTED>(a.d, coarse, tab, lst, a.streams[ui], lane,
                                                 [&](unsigned j) { return !tb_excluded(a.excl, ui, arow, j); }, draws);
    if (lane == 0) a.draws[ui] = draws;

    unsigned p = 1;
    while (p < count) p <<= 1;   // (p <= list_cap; the entries from count on are TB_NONE)
    sn_wave_sort(lst, p, lane);
    unsigned* row = a.items + (size_t)ui * m;
    for (unsigned e = lane; e < m; e += 64) row[e] = lst[e];
    if (lane == 0) a.cnt[ui] = count;
}

// The one scratch allocation of a call: what a chunk of users needs, in bytes from the start.
struct SnLayout {
    size_t chunk_users;      // users per chunk
    size_t excl_cap;         // exclusion indices a chunk may carry
    size_t C, coarse, users, streams, ex_indptr, ex_indices, items, cnt, draws, total;
    SnLayout(size_t n_users, size_t m, size_t dimB, bool weighted)
    {
        n_users = std::max<size_t>(n_users, 1);
        dimB = std::max<size_t>(dimB, 1);
        m = std::max<size_t>(m, 1);
        // the prefix sums (at most 128 MiB), then a quarter of the budget for the exclusion lists -- 2^24 indices, the longest row there
        // is -- and the users' own parts from the rest: stream id, row of A, exclusion row pointer, count, draws and the row itself
        const size_t c_bytes = weighted ? pmf_round_up(dimB * sizeof(unsigned long long), 32) + SN_COARSE * sizeof(unsigned long long) : 0;
        const size_t excl_max = TB_BUDGET / 4 / sizeof(unsigned);
        const size_t per_user = sizeof(unsigned long long) + 4 * sizeof(unsigned) + m * sizeof(unsigned);
        const size_t rest = TB_BUDGET - c_bytes - excl_max * sizeof(unsigned) - 1024;   // (1024: alignment of the nine parts, one spare row pointer)
        chunk_users = std::min({ n_users, TB_CHUNK_USERS_MAX, rest / per_user });
        excl_cap = chunk_users <= excl_max / dimB ? chunk_users * dimB : excl_max;
        TbTake take;
        C = take(weighted ? dimB * sizeof(unsigned long long) : 0);
        coarse = take(weighted ? SN_COARSE * sizeof(unsigned long long) : 0);
        users = take(chunk_users * sizeof(unsigned));
        streams = take(chunk_users * sizeof(unsigned long long));
        ex_indptr = take((chunk_users + 1) * sizeof(unsigned));
        ex_indices = take(excl_cap * sizeof(unsigned));
        items = take(chunk_users * m * sizeof(unsigned));
        cnt = take(chunk_users * sizeof(unsigned));
        draws = take(chunk_users * sizeof(unsigned));
        total = take.o;
    }
};
static_assert(SN_MAX_ITEMS * 8 + SN_COARSE * 8 + TB_BUDGET / 4 + 1024 + 64 * (24 + SN_MAX_M * 4) <= TB_BUDGET, "the smallest chunk holds many of the longest rows");
static_assert(SN_MAX_ITEMS <= TB_BUDGET / 4 / sizeof(unsigned), "the longest exclusion row fits a chunk");

template <int WAVES, bool WEIGHTED> hipError_t sn_launch(const SnArgs& a, hipStream_t stream)
{
    const size_t lds = (WEIGHTED ? SN_COARSE * sizeof(unsigned long long) : 0) + (size_t)WAVES * (((size_t)1 << a.d.log_slots) + a.list_cap) * sizeof(unsigned);
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_negatives_kernel<WAVES, WEIGHTED>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sample_negatives_kernel<WAVES, WEIGHTED>), dim3((unsigned)pmf_ceil_div(a.n_users, WAVES)), dim3(64 * WAVES), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t poismf_hip_sample_negatives_scratch_bytes(size_t n_users, size_t m, size_t dimB, int weighted)
{
    return SnLayout(n_users, m, dimB, weighted != 0).total;
}

extern "C" void poismf_hip_philox4x32(const uint32_t* counter, const uint32_t* key, uint32_t* out) { pmf_philox4x32_10(counter, key, out); }

// The argument checks of both entry points: 0, or 2.  No device call.  n_ids: users must lie below it (0: any id is a stream's).
int poismf_hip_sample_negatives_check(const sparse_ix* users, size_t n_users, size_t m, size_t n_ids, size_t dimB, const sparse_ix* excl_indptr,
                                      const sparse_ix* excl_indices, const uint32_t* item_weight)
{
    if (m < 1 || m > SN_MAX_M || dimB < 1 || dimB > SN_MAX_ITEMS || users == nullptr) return 2;
    for (size_t i = 0; i < n_users; i++) {
        const bool negative = sizeof(sparse_ix) < 8 && (long long)users[i] < 0;   // (int indices; a size_t id may have its top bit set)
        if (negative || (n_ids != 0 && (size_t)users[i] >= n_ids)) return 2;
    }
    if (excl_indptr != nullptr && !tb_rows_ok(excl_indptr, excl_indices, n_users, dimB, TB_BUDGET / 2 / sizeof(unsigned))) return 2;
    if (item_weight != nullptr) {
        unsigned long long W = 0;
        for (size_t j = 0; j < dimB; j++) W += item_weight[j];
        if (W == 0) return 2;
    }
    return 0;
}

// ---- core (tb_batch.hpp) ----
int poismf_hip_sample_negatives_core(hipStream_t stream, size_t dimB, const sparse_ix* users, size_t n_users, size_t m, uint64_t seed,
                                     PmfTopnSeen* seen, const sparse_ix* excl_indptr, const sparse_ix* excl_indices, const uint32_t* item_weight,
                                     void** d_scratch, size_t* scratch_cap, sparse_ix* items, sparse_ix* count, sparse_ix* draws)
{
    if (seen != nullptr && poismf_hip_topn_seen_sorted(*seen, stream)) return 1;
    const bool weighted = item_weight != nullptr;
    const SnLayout L(n_users, m, dimB, weighted);
    TB_TRY(grow_buffer(*d_scratch, *scratch_cap, L.total, 1, stream));
    unsigned char* base = (unsigned char*)*d_scratch;

    SnArgs a = {};
    a.users = (const unsigned*)(base + L.users);
    a.streams = (const unsigned long long*)(base + L.streams);
    a.d = sn_draw_of(m, dimB, seed);
    a.list_cap = m <= SN_SMALL_M ? (unsigned)SN_SMALL_M : 1u << sn_pow2_at_least(m);
    a.items = (unsigned*)(base + L.items);
    a.cnt = (unsigned*)(base + L.cnt);
    a.draws = (unsigned*)(base + L.draws);
    if (weighted) TB_TRY(sn_stage_weights(a.d, item_weight, dimB, base + L.C, base + L.coarse, stream));

    std::vector<unsigned> hu, hp, hx, hix, hc;
    std::vector<unsigned long long> hs;
    for (size_t u0 = 0; u0 < n_users;) {
        size_t u1, nx;
        if (tb_stage_chunk(u1, nx, a.excl, u0, n_users, L.chunk_users, L.excl_cap, excl_indptr, excl_indices, users, false, seen, tb_chunk_dev(base, L), hu, hp,
                           hx, stream))
            return 1;
        const size_t nu = u1 - u0;
        hs.resize(nu);
        for (size_t i = 0; i < nu; i++) hs[i] = (unsigned long long)(size_t)users[u0 + i];
        TB_TRY(pmf_upload(base + L.streams, hs.data(), nu * sizeof(unsigned long long), stream));
        a.n_users = (unsigned)nu;
        if (m <= SN_SMALL_M) TB_TRY((weighted ? sn_launch<4, true>(a, stream) : sn_launch<4, false>(a, stream)));
        else TB_TRY((weighted ? sn_launch<1, true>(a, stream) : sn_launch<1, false>(a, stream)));
        if (tb_fetch_results(u0, nu, m, a.items, nullptr, hix, items, nullptr, stream)) return 1;
        hc.resize(nu);
        TB_TRY(pmf_download(hc.data(), a.cnt, nu * sizeof(unsigned), stream));
        for (size_t i = 0; i < nu; i++) count[u0 + i] = (sparse_ix)hc[i];
        if (draws != nullptr) {
            TB_TRY(pmf_download(hc.data(), a.draws, nu * sizeof(unsigned), stream));
            for (size_t i = 0; i < nu; i++) draws[u0 + i] = (sparse_ix)hc[i];
        }
        u0 = u1;
    }
    return 0;
}

extern "C" {

int poismf_hip_sample_negatives(size_t dimB, const sparse_ix* users, size_t n_users, size_t m, uint64_t seed, const sparse_ix* excl_indptr,
                                const sparse_ix* excl_indices, const uint32_t* item_weight, sparse_ix* items, sparse_ix* count, sparse_ix* draws)
{
    if (n_users == 0) return 0;
    if (items == nullptr || count == nullptr) return 2;
    if (const int rc = poismf_hip_sample_negatives_check(users, n_users, m, 0, dimB, excl_indptr, excl_indices, item_weight)) return rc;
    if (hipSetDevice(pmf_env_device()) != hipSuccess) return 1;
    const hipStream_t st = nullptr;
    void* d_scratch = nullptr;
    size_t scratch_cap = 0;
    const int rc = poismf_hip_sample_negatives_core(st, dimB, users, n_users, m, seed, nullptr, excl_indptr, excl_indices, item_weight, &d_scratch,
                                                    &scratch_cap, items, count, draws);
    pmf_free(d_scratch, st);
    return rc;
}

}  // extern "C"
