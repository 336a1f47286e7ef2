// half_sweep.hip -- issuing a half-sweep on a session: the prologue (column sums of the fixed factor, the padded gather copy), the team
// launches' preparation, the issue loop over the planned launches (planner.hip decides them, the row-kernel units run them), the epilogue
// (join, re-runs of team launches that gave up, the early-stop counter), and the small dense kernels all of that needs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "session.hpp"

#define PMF_EW _Pragma("unroll") for (int i = 0; i < NC; i++)

// ---- compact factor -> line-padded copy (the pad columns stay zero from the allocation) --------------------------
template <class T> __global__ __launch_bounds__(256) void repad_kernel(const T* src, T* dst, size_t n, int k, int ld)
{
    const size_t total = n * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)k;
        const int c = (int)(i - r * (size_t)k);
        dst[r * (size_t)ld + c] = src[i];
    }
}

// ---- column sums of a dense [n x k] factor: sum_by_cols, ref: src/poismf.c:77-83 ---------------------
// stage 1: wave w accumulates rows w, w + nw, ...; stage 2: one wave adds the nw partials in order,
// then applies `+ l1` (ref: :513-514) and the PG pre-scalings (ref: :523-526, :573-577, quirk Q1).
// stage 1: blocks of 8 waves; wave w of block b accumulates rows (b*8 + w), + 8*grid, ...; the 8 wave totals are added
// through LDS in wave order, so the 256-way partial written by the block is bit-reproducible.
constexpr int COLSUM_BLOCK_WAVES = 8;
template <class T, int NC>
__global__ __launch_bounds__(WAVE* COLSUM_BLOCK_WAVES) void colsum_partial_kernel(const T* M, size_t n, int k, T* partial, unsigned block0, unsigned nblocks)
{
    // (block0 / nblocks: this launch computes blocks [block0, block0 + gridDim.x) of the nblocks the whole sum is cut into -- a block's
    // partial sum depends on nblocks and on its own number alone, so ANY subset of blocks, computed anywhere, gives the same bits: what lets
    // the ranks of a multi-GPU run share the first stage, poismf_hip_session_colsum_partial)
    __shared__ T part[COLSUM_BLOCK_WAVES][NC * WAVE];
    const int lane = lane_id();
    const int w = (int)(threadIdx.x / WAVE);
    T acc[NC];
    PMF_EW acc[i] = (T)0;
    // four rows in flight per wave (the loop is latency-bound: one 200-byte row per trip); added in row order as before
    const unsigned bid = blockIdx.x + block0;
    const size_t stride = (size_t)nblocks * COLSUM_BLOCK_WAVES;
    size_t r = (size_t)bid * COLSUM_BLOCK_WAVES + w;
    for (; r + 3 * stride < n; r += 4 * stride) {
        T v[4][NC];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const T* row = M + (r + u * stride) * (size_t)k;
            PMF_EW v[u][i] = (lane + WAVE * i < k) ? row[lane + WAVE * i] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) { PMF_EW acc[i] += v[u][i]; }
    }
    for (; r < n; r += stride) {
        const T* row = M + r * (size_t)k;
        PMF_EW if (lane + WAVE * i < k) acc[i] += row[lane + WAVE * i];
    }
    PMF_EW part[w][lane + WAVE * i] = acc[i];
    __syncthreads();
    if (w == 0) {
        PMF_EW {
            const int c = lane + WAVE * i;
            if (c < k) {
                T s = part[0][c];
                for (int q = 1; q < COLSUM_BLOCK_WAVES; q++) s += part[q][c];
                partial[(size_t)bid * k + c] = s;
            }
        }
    }
}
// stage 2: 16 waves; wave w adds partials w, w + 16, ... in order, then wave 0 adds the 16 wave totals in order
// (fixed summation order => bit-reproducible), applies `+ l1` and the PG pre-scalings.
constexpr int COLSUM_FINAL_WAVES = 16;
template <class T, int NC>
__global__ __launch_bounds__(WAVE* COLSUM_FINAL_WAVES) void colsum_final_kernel(const T* partial, int nw, int k, T l1, T scale,
                                                                                 int nscale, T* out)
{
    __shared__ T part[COLSUM_FINAL_WAVES][NC * WAVE];
    const int lane = lane_id();
    const int w = (int)(threadIdx.x / WAVE);
    T acc[NC];
    PMF_EW acc[i] = (T)0;
    int r = w;
    for (; r + 7 * COLSUM_FINAL_WAVES < nw; r += 8 * COLSUM_FINAL_WAVES) {   // eight loads in flight, same order of adds
        T v[8][NC];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            PMF_EW v[u][i] = (lane + WAVE * i < k) ? partial[(size_t)(r + u * COLSUM_FINAL_WAVES) * k + lane + WAVE * i] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) { PMF_EW acc[i] += v[u][i]; }
    }
    for (; r < nw; r += COLSUM_FINAL_WAVES) {
        PMF_EW if (lane + WAVE * i < k) acc[i] += partial[(size_t)r * k + lane + WAVE * i];
    }
    PMF_EW part[w][lane + WAVE * i] = acc[i];
    __syncthreads();
    if (w == 0) {
        PMF_EW {
            const int c = lane + WAVE * i;
            if (c < k) {
                T s = part[0][c];
                for (int q = 1; q < COLSUM_FINAL_WAVES; q++) s += part[q][c];
                if (l1 > (T)0.) s += l1;
                for (int q = 0; q < nscale; q++) s *= scale;
                out[c] = s;
            }
        }
    }
}

// column-sum kernels: elements per lane in the plain lane <-> element layout
int nc_for_k(size_t k) { return k <= 64 ? 1 : (k <= 128 ? 2 : (k <= 256 ? 4 : (k <= 512 ? 8 : 0))); }

namespace {

inline int colsum_blocks_for(const poismf_hip_session* s, size_t n)
{
    return (int)std::min<size_t>((size_t)s->colsum_waves, std::max<size_t>((n + COLSUM_BLOCK_WAVES - 1) / COLSUM_BLOCK_WAVES, 1));
}
template <int NC> int launch_colsum_partial(poismf_hip_session* s, const real_t* M, size_t n, int b_lo, int b_hi)
{
    const int nw = colsum_blocks_for(s, n);
    if (b_lo < 0 || b_hi > nw || b_lo > b_hi) return 1;
    s->partials_of = M;
    s->partials_given = false;
    if (b_hi > b_lo)
        hipLaunchKernelGGL((colsum_partial_kernel<real_t, NC>), dim3(b_hi - b_lo), dim3(WAVE * COLSUM_BLOCK_WAVES), 0, s->stream, M, n, (int)s->k,
                           s->d_partial, (unsigned)b_lo, (unsigned)nw);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <int NC> int launch_colsum(poismf_hip_session* s, const real_t* M, size_t n, real_t l1, real_t scale, int nscale)
{
    const int nw = colsum_blocks_for(s, n);
    // first stage: all blocks here, or only [b_lo, b_hi) (the others are the peers' and have been put into d_partial by the caller), or none
    int b_lo = 0, b_hi = nw;
    if (s->partials_given && s->partials_of == M) { b_lo = b_hi = 0; }
    s->partials_given = false;        // (one shot, whoever consumes or declines it)
    if (b_hi > b_lo)
        hipLaunchKernelGGL((colsum_partial_kernel<real_t, NC>), dim3(b_hi - b_lo), dim3(WAVE * COLSUM_BLOCK_WAVES), 0, s->stream, M, n, (int)s->k,
                           s->d_partial, (unsigned)b_lo, (unsigned)nw);
    hipLaunchKernelGGL((colsum_final_kernel<real_t, NC>), dim3(1), dim3(WAVE * COLSUM_FINAL_WAVES), 0, s->stream, s->d_partial, nw, (int)s->k, l1,
                       scale, nscale, s->d_bsum);
    HIP_TRY(hipGetLastError());
    return 0;
}

int colsum_partial(poismf_hip_session* s, const real_t* M, size_t n, int b_lo, int b_hi)
{
    switch (nc_for_k(s->k)) {
        case 1: return launch_colsum_partial<1>(s, M, n, b_lo, b_hi);
        case 2: return launch_colsum_partial<2>(s, M, n, b_lo, b_hi);
        case 4: return launch_colsum_partial<4>(s, M, n, b_lo, b_hi);
        case 8: return launch_colsum_partial<8>(s, M, n, b_lo, b_hi);
    }
    return 1;
}
int colsum(poismf_hip_session* s, const real_t* M, size_t n, real_t l1, real_t scale, int nscale)
{
    switch (nc_for_k(s->k)) {
        case 1: return launch_colsum<1>(s, M, n, l1, scale, nscale);
        case 2: return launch_colsum<2>(s, M, n, l1, scale, nscale);
        case 4: return launch_colsum<4>(s, M, n, l1, scale, nscale);
        case 8: return launch_colsum<8>(s, M, n, l1, scale, nscale);
    }
    return 1;
}

// ---- a team launch that gives up must not cost the fit (reg_eval.hpp, M_ > 1: an exchange between CUs timed out) -----------
// The rows the team launches of a half cover are saved BEFORE the half's first launch (empty chip); AFTER its last launch has ended, every team
// launch whose error word is set has its rows put back and run again on the streamed LDS kernel (both gated on that word), and one fold kernel
// settles the counters.  Rounds 2-5 bracketed every team launch with these kernels on the launch's own stream: each of them then queued for a
// wave slot behind the other stream's persistent 512-register workgroups (round 5's profile: a restore kernel whose body is one compare, 13 ms
// on average, 8 per C5 sweep) and held the next team launch back.  Now a team launch is ONE dispatch and the healthy case pays its
// bookkeeping where nothing else is resident.
__global__ __launch_bounds__(256) void team_save_rows_kernel(const real_t* M, const RowDesc* desc, unsigned nrows, unsigned row_offset, int k, real_t* backup,
                                                             const unsigned* eval_rows, unsigned* eval_backup)
{
    const size_t n = (size_t)nrows * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)k, c = i % (size_t)k;
        backup[i] = M[(size_t)(row_offset + desc[r].lrow) * (size_t)k + c];
        if (eval_rows != nullptr && c == 0) eval_backup[r] = eval_rows[desc[r].lrow];
    }
}
__global__ __launch_bounds__(256) void team_restore_rows_kernel(real_t* M, real_t* Mp, int ldM, const RowDesc* desc, unsigned nrows, unsigned row_offset,
                                                                int k, const real_t* backup, const unsigned* err, unsigned* eval_rows, const unsigned* eval_backup)
{
    if (*err == 0) return;
    const size_t n = (size_t)nrows * (size_t)k;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)k, c = i % (size_t)k;
        const size_t row = (size_t)(row_offset + desc[r].lrow);
        M[row * (size_t)k + c] = backup[i];
        if (Mp != nullptr) Mp[row * (size_t)ldM + c] = backup[i];
        if (eval_rows != nullptr && c == 0) eval_rows[desc[r].lrow] = eval_backup[r];
    }
}
// After the re-runs: a launch that gave up is counted ([0]) and its own tally of unchanged rows dropped (its re-run counted them again, straight
// into the half's counter, ref: src/poismf.c:393-403); a launch that kept its results adds its tally.  The per-launch words are left zeroed.
__global__ void team_fold_kernel(unsigned* err, int n, unsigned* n_unchanged)
{
    for (int i = 0; i < n; i++) {
        if (err[2 + i] != 0) err[0] += 1;
        else if (n_unchanged != nullptr) *n_unchanged += err[2 + TEAM_LAUNCH_MAX + i];
        err[2 + i] = 0;
        err[2 + TEAM_LAUNCH_MAX + i] = 0;
    }
}

// The hold-back of a half-sweep's other bins behind its forked long-row launch (poismf_hip_half_sweep): one wave that returns when `goal`
// workgroups of that launch have counted themselves in -- or when `budget` ticks of the constant-rate wall clock have passed, whichever is
// first.  A BOUNDED wait on purpose: rounds 3-4a held the stream with hipStreamWaitValue32, and under `rocprofv3 --pmc` (dispatches serialised
// by the tool) that wait kept the long-row launch from ever starting -- a counter pass over config C5 sat there until gpurun's limit
// (one hour of round 4's GPU time).  This kernel gives up after 2 ms and the bins then run one after the other.
__global__ void hold_back_gate_kernel(const unsigned* word, unsigned goal, unsigned long long budget)
{
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < goal) {
        if (wall_clock64() - t0 > budget) break;
        __builtin_amdgcn_s_sleep(64);
    }
}

// ---- a half-sweep: prologue, plan, team preparation, issue, epilogue ------------------------------------------------
// A team launch's share of the session's team buffers (prepare_teams), in launch order.
struct TeamSlot { size_t backup_at, eval_at; int area; };
// What a team launch becomes if it gives up: its rows on the streamed LDS kernel, gated on its error word, issued after the join.
struct TeamRerun { HalfArgs<real_t> af; OneLaunch of; size_t slot; };

bool is_team(Engine e) { return e == Engine::RegTeam || e == Engine::LaneTeam || e == Engine::Giant; }
bool is_long(Engine e) { return e == Engine::LdsLong || e == Engine::Giant; }   // a workgroup of LONG_NW waves per row, on the long stream

// The stream a launch runs on: `bin` is the balanced stream of the one-wave bins, `longs` the one the long rows share.  (PG has no one-wave
// Lane launch -- lane_shape_for gives it four-wave shapes only -- so every one-wave Lane launch is CG's, TNCG's or the evaluation kernels'.)
hipStream_t launch_stream(const PlannedLaunch& L, hipStream_t main, hipStream_t bin, hipStream_t longs)
{
    switch (L.engine) {
        case Engine::Reg: case Engine::Lds: return bin;
        case Engine::Lane: return L.nw == 1 ? bin : main;
        case Engine::RegW: case Engine::RegTeam: return main;
        case Engine::LaneTeam: case Engine::LdsLong: case Engine::Giant: return longs;
    }
    return main;
}

// The half's prologue: column sums of the fixed factor (or the caller's k-vector), the padded gather copy, and the arguments every launch of
// the half starts from.
int half_prologue(poismf_hip_session* s, int which, const Half& h, bool subset, const poismf_hip_params* p, real_t step_size, real_t cnst_div,
                  bool prologue, bool early_stop, const real_t* bsum_override, real_t neg_step_override, real_t neg_step2, HalfArgs<real_t>& a)
{
    real_t* M = which ? s->dA : s->dB;
    const real_t* F = which ? s->dB : s->dA;
    const size_t dimF = which ? s->dimB : s->dimA;
    const bool is_pg = p->method == POISMF_PG;

    // column sums of the fixed factor (+ l1), with the PG pre-scaling when w == 1:
    //   B half: * (-step)            ref: src/poismf.c:523-524
    //   A half: * (-step) twice      ref: src/poismf.c:573-577 (quirk Q1)
    real_t neg_step = -step_size;
    if (bsum_override != nullptr) {
        s->partials_given = false;   // (declared for a half that computes its own sum: not for a later one)
        neg_step = neg_step_override;
        HIP_TRY(pmf_upload(s->d_bsum, bsum_override, s->k * sizeof(real_t), s->stream));
    } else if (prologue) {
        int nscale = 0;
        if (is_pg && p->w_mult == (real_t)1.) nscale = which ? 2 : 1;
        if (colsum(s, F, dimF, p->l1_reg, neg_step, nscale)) return 1;
    }

    // the gathers read the line-padded copy of the fixed factor when the session keeps one
    const real_t* Fg = F;
    real_t* Mp = nullptr;
    if (s->ld != 0) {
        // The padded copy of F is current only if this session's own previous half-sweep rewrote ALL of F (its row
        // kernels store every updated row to both copies).  Anything else -- factors set by the caller, a shard
        // exchange between GPUs writing into the compact factor -- is picked up by re-padding the whole factor.
        real_t* Fp = which ? s->dBp : s->dAp;
        if (prologue && !s->padded_fresh[which ? 0 : 1]) {
            const size_t total = dimF * s->k;
            const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)s->num_cu * 16);
            if (blocks > 0) hipLaunchKernelGGL((repad_kernel<real_t>), dim3(blocks), dim3(256), 0, s->stream, F, Fp, dimF, (int)s->k, (int)s->ld);
            HIP_TRY(hipGetLastError());
        }
        Fg = Fp;
        Mp = which ? s->dAp : s->dBp;
        if (prologue) {
            s->padded_fresh[which ? 0 : 1] = true;   // the copy of F was just re-derived (or was current)
            // (a call over listed rows leaves the moving factor's copy as fresh as it was: its row kernels store every row they update to
            // both copies and touch no other -- it can never MAKE the copy fresh)
            if (!subset) s->padded_fresh[which ? 1 : 0] = h.row_begin == 0 && h.row_end == h.dimM;
        }
    }

    a = HalfArgs<real_t>{};
    a.M = M; a.F = Fg;
    a.Mp = Mp; a.ldM = (int)s->ld;
    a.indptr = h.d_indptr; a.indices = h.d_indices; a.values = h.d_values; a.perm = h.d_perm; a.desc = h.d_desc;
    a.row_offset = (unsigned)h.row_begin;
    a.bsum = s->d_bsum;
    a.P.l2 = p->l2_reg; a.P.w = p->w_mult;
    a.P.step = step_size * p->w_mult;  // ref: src/poismf.c:151
    a.P.cnst_div = cnst_div;
    a.P.neg_step = neg_step;
    a.P.neg_step2 = neg_step2;
    a.P.maxupd = (int)std::min<size_t>(p->maxupd, 0x7fffffff);
    a.P.limit_step = p->limit_step;
    a.P.max_cg_it = (int)std::max(1.0, std::min(50.0, (double)(real_t)s->k / 2.0));  // ref: src/poismf.c:342
    // (w_mult > 0: the bound that lets a line search skip a trial needs the data term -w sum x log(.) to be CONVEX along the line;
    // the reference's Python wrapper asserts weight_mult > 0, the C ABI does not)
    a.P.x_pos = (h.x_positive && !plan_knobs().no_ls_prune && p->w_mult > (real_t)0) ? 1 : 0;
    a.reuse_prev = p->reuse_prev;
    a.early_stop = early_stop;
    a.n_unchanged = s->d_counter;
    a.stop = is_pg ? nullptr : device_stop_word();   // (pinned host memory, portable: the same address on every device)
    a.eval_rows = s->profiling ? h.d_eval_rows : nullptr;
    a.dec_rows = s->profiling ? h.d_dec_rows : nullptr;
    a.team_err = s->d_team_err + 2;
    a.team_spin = plan_knobs().team_spin;
    a.team_members = 1;
    if (a.early_stop && prologue) HIP_TRY(hipMemsetAsync(s->d_counter, 0, sizeof(unsigned), s->stream));
    return 0;
}

// Everything the team launches of a half need, once, on the main stream, before anything of the half is on the chip: a zeroed buffer area,
// row-queue head (+ one for the re-run), error word and tally per launch, and a copy of the rows they start from.
int prepare_teams(poismf_hip_session* s, const Half& h, const HalfArgs<real_t>& base, const std::vector<PlannedLaunch>& launches,
                  std::vector<TeamSlot>& tslots)
{
    size_t elems = 0, rows = 0;
    int n_gt = 0, n_reg = 0;
    for (const PlannedLaunch& L : launches) {
        if (!is_team(L.engine)) continue;
        const bool gt = L.engine != Engine::RegTeam;   // lane teams and giant rows share the GT_* layout
        tslots.push_back({ elems, rows, gt ? n_gt++ : n_reg++ });
        elems += (size_t)L.count * s->k;
        rows += L.count;
    }
    if (tslots.empty()) return 0;
    // (sized for the whole half at once)
    HIP_TRY(grow_buffer(s->d_gt, s->gt_areas, (size_t)n_gt, (size_t)GT_BUF_BYTES, s->stream));
    HIP_TRY(grow_buffer(s->d_team, s->team_areas, (size_t)n_reg, (size_t)TEAM_BUF_BYTES, s->stream));
    HIP_TRY(grow_buffer(s->d_team_backup, s->team_backup_elems, elems, sizeof(real_t), s->stream));
    if (base.eval_rows != nullptr) HIP_TRY(grow_buffer(s->d_team_eval_backup, s->team_eval_backup_rows, rows, sizeof(unsigned), s->stream));
    // (a giant / lane team's area is used up to its teams' words: the whole areas are zeroed all the same -- n x 4.6 MB, microseconds on an
    // empty chip, where round 5 zeroed one area per launch between persistent kernels)
    if (n_gt) HIP_TRY(hipMemsetAsync(s->d_gt, 0, (size_t)n_gt * (size_t)GT_BUF_BYTES, s->stream));
    if (n_reg) HIP_TRY(hipMemsetAsync(s->d_team, 0, (size_t)n_reg * (size_t)TEAM_BUF_BYTES, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_queue + MAX_LAUNCHES, 0, sizeof(unsigned) * 2 * TEAM_LAUNCH_MAX, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_team_err + 2, 0, sizeof(unsigned) * 2 * TEAM_LAUNCH_MAX, s->stream));
    size_t ti = 0;
    for (const PlannedLaunch& L : launches) {
        if (!is_team(L.engine)) continue;
        const size_t need = (size_t)L.count * s->k;
        hipLaunchKernelGGL(team_save_rows_kernel, dim3((unsigned)std::min<size_t>((need + 255) / 256, (size_t)s->num_cu * 8)), dim3(256), 0, s->stream,
                           base.M, h.d_desc + L.begin, L.count, (unsigned)h.row_begin, (int)s->k, s->d_team_backup + tslots[ti].backup_at,
                           (const unsigned*)base.eval_rows, base.eval_rows != nullptr ? s->d_team_eval_backup + tslots[ti].eval_at : nullptr);
        ti++;
    }
    HIP_TRY(hipGetLastError());
    s->team_launched = true;
    return 0;
}

// If team launch `slot` (launched as o with arguments a) gives up: its rows back to where they started, the same rows on the streamed LDS
// kernel -- one wave per row for register teams, eight for giant rows and lane teams -- after the join.
TeamRerun team_rerun(const poismf_hip_session* s, const PlannedLaunch& L, const OneLaunch& o, const HalfArgs<real_t>& a, size_t slot)
{
    const bool eight = L.engine != Engine::RegTeam;
    HalfArgs<real_t> af = a;
    // (a.geom is the LDS engine's geometry for the launch's longest length class: what these rows take without teams -- but a lane team carries the
    // one-wave geometry of its class: the eight-wave streamed kernel wants its own)
    if (L.engine == Engine::LaneTeam) af.geom = long_geom(af.geom);
    af.team_buf = nullptr; af.gate = a.team_err; af.arrive = nullptr; af.n_unchanged = s->d_counter;
    af.queue = s->d_queue + MAX_LAUNCHES + TEAM_LAUNCH_MAX + slot;
    OneLaunch of = o;
    of.engine = eight ? Engine::LdsLong : Engine::Lds;
    of.reg_S = 0; of.nw = eight ? LONG_NW : 1; of.team = 0; of.lane = LaneShape{};
    of.s_load = af.geom.s_load; of.stream = s->stream;
    of.lds = lds_bytes_per_block(af.geom, sizeof(real_t), of.nw);
    of.grid = eight ? (unsigned)std::min<size_t>(L.count, (size_t)s->num_cu)
                    : (unsigned)std::min<size_t>(L.count, (size_t)s->num_cu * std::max<size_t>(1, std::min<size_t>(16, LDS_PER_CU / of.lds)) * 2);
    return { af, of, slot };
}

// Issues the half's launches in plan order: per launch its arguments, grid, stream, the hold-back gate behind a long-row launch and, in
// profiling sessions, events around it.  The re-runs of the team launches are described in `reruns`, not issued.
int issue_half(poismf_hip_session* s, int which, int method, const std::vector<PlannedLaunch>& launches, const HalfArgs<real_t>& base,
               const std::vector<TeamSlot>& tslots, bool dynamic, bool forked, std::vector<TeamRerun>& reruns)
{
    // (two TEAM launches must never run beside each other: each waits for partners that need the CUs the other's partial teams hold -- giant rows
    // and lane teams follow one another on the SECOND stream, beside the main stream's non-team bins)
    const hipStream_t long_stream = forked ? s->aux_stream : s->stream;
    double queued[2] = { 0.0, 0.0 };
    unsigned arrive_goal = 0;
    size_t team_no = 0;
    for (size_t i = 0; i < launches.size(); i++) {
        const PlannedLaunch& L = launches[i];
        const std::string name = launch_name(method, L);
        s->last_plan[which] += plan_item(method, L);
        HalfArgs<real_t> a = base;
        a.perm_begin = L.begin; a.nrows = L.count; a.geom = L.geom;
        a.team_members = (unsigned)std::max(1, L.team);
        // Waves launched per resident wave slot.  Rows pulled from the queue balance themselves: 2 is enough.  Rows dealt
        // out statically come in nnz-descending order, so wave 0 always gets the longest of each round; many short
        // waves let the dispatcher even that out (measured on C2, PG(10): 2 -> 1.214 ms, 8 -> 1.165, 32 -> 1.146).
        // The single-wave register kernels are always dealt out this way: with ~1 row per wave the hardware dispatcher IS
        // the queue (CG fp32 on C2: 3.87 ms with tickets, 3.35 ms without).
        const bool one_wave = L.engine == Engine::Reg || (L.engine == Engine::Lane && L.nw == 1);
        a.queue = dynamic && !one_wave ? s->d_queue + i : nullptr;
        unsigned grid_mult = one_wave ? 32 : 2;
        // PG on the multi-wave lane kernel: ONE ROW PER WORKGROUP, the hardware dispatcher hands them out.  C4 matrix, PG(10), the 78 715 item
        // rows of 513 .. 1024 nonzeros: persistent workgroups walking rows r, r + grid, .. at 2 / 4 / 8 / 16 / 64 workgroups per slot 4.28 /
        // 4.13 / 4.08 / 4.09 / 4.39 ms; persistent workgroups on the queue 4.07; one row per workgroup 3.87 ms.  The queue's gain is balance
        // (no workgroup owns a fixed share of the rows); what the dispatcher gains on top is measured, not explained (DESIGN.md section 6.0:
        // neither the cross-row pipeline nor start delays account for it; the workgroup-wide ticket's two barriers per row remain).
        // (Not for CG / TNCG, whose rows differ in cost and want the longest-first queue: CG fp32 B half 11.25 -> 13.17 ms; not for the
        // eight-wave register kernel, one workgroup per CU: 1.83 -> 1.90.)
        if (method == POISMF_PG && L.engine == Engine::Lane && L.nw > 1) grid_mult = 1u << 20;
        const size_t lds = lds_bytes_per_block(a.geom, sizeof(real_t), L.nw);
        const unsigned waves_per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(16, LDS_PER_CU / lds));
        unsigned grid = (unsigned)std::min<size_t>(L.count, (size_t)s->num_cu * waves_per_cu * grid_mult);
        if (L.engine == Engine::Giant)   // whole teams only: as many as the chip holds at one workgroup per CU
            grid = std::max(1u, std::min((unsigned)L.count, std::min((unsigned)GT_TEAMS_MAX, (unsigned)s->num_cu / (unsigned)GT_M))) * (unsigned)GT_M;
        if (L.engine == Engine::LaneTeam)   // whole teams, one workgroup per CU
            grid = std::max(1u, std::min((unsigned)L.count, (unsigned)s->num_cu / (unsigned)L.team)) * (unsigned)L.team;
        a.arrive = forked && is_long(L.engine) ? s->d_arrive : nullptr;
        const size_t slot = team_no;
        if (is_team(L.engine)) {
            // one dispatch: its queue head, buffer area, error word and tally are its own and were zeroed before the half began
            team_no++;
            a.queue = s->d_queue + MAX_LAUNCHES + slot;                     // teams always draw their rows from a queue
            a.team_err = s->d_team_err + 2 + slot;
            a.n_unchanged = s->d_team_err + 2 + TEAM_LAUNCH_MAX + slot;   // kept only if the launch's results are (team_fold_kernel)
            a.team_buf = L.engine == Engine::RegTeam ? s->d_team + (size_t)tslots[slot].area * (size_t)(TEAM_BUF_BYTES / 8)
                                                     : s->d_gt + (size_t)tslots[slot].area * (size_t)(GT_BUF_BYTES / 8);
        }
        // (with long rows on the second stream, the one-wave bins that follow go wherever less work is queued -- unless the half has TEAM launches:
        // they follow one another on the second stream and are the half's critical path; round 6's timeline of a C5 sweep, profiles/r06/kt_c5_timeline.txt,
        // showed the last one-wave bin queued behind all seven of them and running alone for 8 ms after the main stream had been idle for 33)
        // (multi-wave launches count against the second stream wherever they are issued)
        const int lane_stream = (forked && tslots.empty() && L.nw == 1 && queued[1] < queued[0]) ? 1 : 0;
        queued[L.nw > 1 ? 1 : lane_stream] += (double)L.count * (double)std::max(16, L.reg_S > 0 ? L.reg_S * REG_JG : L.geom.cap);
        OneLaunch o = L;
        o.stream = launch_stream(L, s->stream, lane_stream ? s->aux_stream : s->stream, long_stream);
        o.lds = lds; o.grid = grid; o.grid_mult = grid_mult;
        o.device = s->device; o.num_cu = s->num_cu;
        LaunchRec lr{};
        if (s->profiling) {   // events around this launch, on its stream
            HIP_TRY(hipEventCreate(&lr.t0));
            HIP_TRY(hipEventCreate(&lr.t1));
            lr.which = which; lr.name = name; lr.rows = L.count; lr.nnz = L.nnz;
            HIP_TRY(hipEventRecord(lr.t0, o.stream));
        }
        const int rc = pmf_launch_one(method, o, a);
        if (!rc && a.arrive != nullptr) {
            arrive_goal += std::min<unsigned>(grid, (unsigned)s->num_cu);   // (one eight-wave workgroup per CU)
            // (hold_back_gate_kernel: returns when that many workgroups are on the chip, or after 2 ms)
            hipLaunchKernelGGL(hold_back_gate_kernel, dim3(1), dim3(1), 0, s->stream, s->d_arrive, arrive_goal, s->gate_budget);
        }
        if (!rc && is_team(L.engine)) reruns.push_back(team_rerun(s, L, o, a, slot));
        if (s->profiling) {
            HIP_TRY(hipEventRecord(lr.t1, o.stream));
            s->lprof.push_back(lr);
        }
        if (rc) return 1;
    }
    return 0;
}

// A pass's epilogue: the join; per team launch a restore and a streamed re-run that return at once unless the launch's error word is set,
// then the fold -- on a chip that has nothing else resident; the early-stop counter.
int half_epilogue(poismf_hip_session* s, const Half& h, int method, const HalfArgs<real_t>& base, bool forked, const std::vector<TeamSlot>& tslots,
                  const std::vector<TeamRerun>& reruns, const ProfRec* rec, size_t* n_unchanged)
{
    if (forked) {
        HIP_TRY(hipEventRecord(s->ev_join, s->aux_stream));
        HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_join, 0));
    }
    for (const TeamRerun& r : reruns) {
        hipLaunchKernelGGL(team_restore_rows_kernel, dim3((unsigned)std::min<size_t>(((size_t)r.af.nrows * s->k + 255) / 256, (size_t)s->num_cu * 8)),
                           dim3(256), 0, s->stream, base.M, base.Mp, (int)s->ld, h.d_desc + r.af.perm_begin, r.af.nrows, (unsigned)h.row_begin, (int)s->k,
                           s->d_team_backup + tslots[r.slot].backup_at, s->d_team_err + 2 + r.slot, base.eval_rows,
                           base.eval_rows != nullptr ? s->d_team_eval_backup + tslots[r.slot].eval_at : nullptr);
#ifndef PMF_LANE_ONLY   // (development builds without the streamed kernels: no re-run)
        if (pmf_launch_one(method, r.of, r.af)) return 1;
#endif
    }
    if (!reruns.empty()) {
        hipLaunchKernelGGL(team_fold_kernel, dim3(1), dim3(1), 0, s->stream, s->d_team_err, (int)tslots.size(), base.early_stop ? s->d_counter : nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (rec != nullptr) {   // (the call's last pass)
        HIP_TRY(hipEventRecord(rec->t1, s->stream));
        s->prof.push_back(*rec);
    }
    if (base.early_stop && n_unchanged != nullptr) {
        unsigned cnt = 0;
        HIP_TRY(pmf_download(&cnt, s->d_counter, sizeof(unsigned), s->stream));
        *n_unchanged = cnt;
    }
    return 0;
}

}  // namespace

// Team launches (reg_eval.hpp, M_ > 1) give up instead of hanging when an exchange between CUs times out; the word they set
// is read where the session synchronises anyway.  Nonzero: the factors are not to be trusted.
int team_check(poismf_hip_session* s)
{
    if (!s->team_launched) return 0;
    unsigned w[2] = { 0, 0 };
    HIP_TRY(pmf_download(w, s->d_team_err, 2 * sizeof(unsigned), s->stream));
    s->team_launched = false;
    if (w[0] != 0) {
        // (somebody else holds CUs: every further team launch would sit out its time-out as well -- 300 ms each, up to eight per half on config C5.
        // The rest of this session plans without teams: the rows take the streamed kernels directly, which is what a re-run gives them anyway.)
        s->teams_off = true;
        fprintf(stderr, "poismf_hip: %u multi-CU row launch(es) timed out waiting for a partner CU and were re-run on the streamed path "
                        "(results are valid; another process or kernel is holding CUs; no further multi-CU launches in this session)\n", w[0]);
        HIP_TRY(hipMemsetAsync(s->d_team_err, 0, 2 * sizeof(unsigned), s->stream));
    }
    return 0;
}

// bsum_override != nullptr: use this HOST k-vector (already carrying l1 and any PG scaling) instead of the column
// sums of the fixed factor; neg_step_override then replaces -step_size as the PG scale of the per-row Bsum_w.
// seg < 0: every segment of the shard, one pass after the other (plan_call); seg >= 0: that segment only -- segment 0 then also runs the
// prologue (column sums, refresh of the padded gather copy, reset of the early-stop counter), and the counter is read by whichever call
// passes n_unchanged (the last segment).  Either way a segment's launches are the same launches.
// view != nullptr: a half that shares the session half's matrix arrays and has a permutation, descriptors and bins of its own over SOME of
// its rows (poismf_hip_half_sweep_rows) -- everything below runs on it as it runs on the whole half.
int half_sweep_impl(poismf_hip_session* s, int which, const poismf_hip_params* p, real_t step_size, real_t cnst_div,
                           size_t* n_unchanged, const real_t* bsum_override, real_t neg_step_override, real_t neg_step2,
                           int seg, const Half* view)
{
    HIP_TRY(hipSetDevice(s->device));
    which = which ? 1 : 0;
    const Half& h = view != nullptr ? *view : s->half[which];
    if (seg >= (int)h.segs.size()) return 1;
    const bool early_stop = (p->method == POISMF_TNCG) && p->early_stop && (n_unchanged != nullptr || seg >= 0);
    const bool is_pg = p->method == POISMF_PG;
    const PlanCtx c = plan_ctx(s->k, which ? s->dimB : s->dimA, p->method, p->maxupd, p->w_mult, p->limit_step != 0, s->teams_off, s->num_cu);
    const std::vector<std::vector<PlannedLaunch>> passes = plan_call(h.segs, seg, c);
    ProfRec rec{};
    for (size_t i = 0; i < passes.size(); i++) {
        const std::vector<PlannedLaunch>& launches = passes[i];
        const bool prologue = seg <= 0 && i == 0, last = i + 1 == passes.size();
        HalfArgs<real_t> base;
        if (half_prologue(s, which, h, view != nullptr, p, step_size, cnst_div, prologue, early_stop, bsum_override, neg_step_override, neg_step2, base))
            return 1;
        if (s->profiling && i == 0) {
            HIP_TRY(hipEventCreate(&rec.t0));
            HIP_TRY(hipEventCreate(&rec.t1));
            rec.which = which;
            HIP_TRY(hipEventRecord(rec.t0, s->stream));
        }
        // (every team launch of a pass has a row-queue head, an error word, a tally and a buffer area of its own: the session holds
        // TEAM_LAUNCH_MAX of each.  A segment has one team launch per team shape, eight at most; a plan with more is refused, never re-planned)
        if (std::count_if(launches.begin(), launches.end(), [](const PlannedLaunch& L) { return is_team(L.engine); }) > TEAM_LAUNCH_MAX) {
            fprintf(stderr, "poismf_hip: a half-sweep pass with more than %d multi-CU row launches\n", TEAM_LAUNCH_MAX);
            pmf_last_hip_error() = hipErrorInvalidValue;
            return 1;
        }
        const bool dynamic = !is_pg && !plan_knobs().static_rows && launches.size() <= (size_t)MAX_LAUNCHES;
        // (PG's multi-wave lane launches take ONE ROW PER WORKGROUP, issue_half; persistent workgroups on the queue or with static shares -- rounds 2-4a,
        // POISMF_HIP_PG_LANE_ROWS -- lost to it, DESIGN.md 6.0, and went in round 6)
        if (dynamic) HIP_TRY(hipMemsetAsync(s->d_queue, 0, sizeof(unsigned) * MAX_LAUNCHES, s->stream));
        // The few workgroup-per-row launches of the power-law tail occupy a few dozen CUs for a long time: run them on a second stream beside the
        // other bins (fork after the column sums, join before anything reads the result) -- NEXT TO the other bins, not after them.  The other bins'
        // kernels are persistent (a workgroup keeps its CU until the bin's queue is empty): whichever kernel reaches the chip first fills it, and on
        // config C5 that was the mid-length bin -- the 60 giant rows then waited 260 ms for a CU and ran on their own afterwards (390 ms for what
        // takes 150 alone).  So every workgroup of a long-row launch counts itself in when it starts, and the main stream waits for that count (a
        // one-wave gate kernel with a time limit; rounds 3-4a: hipStreamWaitValue32) before it launches anything else.  Arrivals only ever grow, so
        // a chip that cannot hold the whole launch at once delays the main stream by the gate's 2 ms, no more.
        const bool forked = !plan_knobs().no_fork && launches.size() > 1 &&
                            std::any_of(launches.begin(), launches.end(), [](const PlannedLaunch& L) { return is_long(L.engine); });
        if (forked) HIP_TRY(hipMemsetAsync(s->d_arrive, 0, sizeof(unsigned), s->stream));
        std::vector<TeamSlot> tslots;
        if (prepare_teams(s, h, base, launches, tslots)) return 1;
        if (forked) {
            HIP_TRY(hipEventRecord(s->ev_fork, s->stream));
            HIP_TRY(hipStreamWaitEvent(s->aux_stream, s->ev_fork, 0));
        }
        if (prologue) s->last_plan[which].clear();
        std::vector<TeamRerun> reruns;
        if (issue_half(s, which, p->method, launches, base, tslots, dynamic, forked, reruns)) return 1;
        if (half_epilogue(s, h, p->method, base, forked, tslots, reruns, s->profiling && last ? &rec : nullptr, last ? n_unchanged : nullptr)) return 1;
    }
    return 0;
}

extern "C" {

// ---- the first stage of the column sums, shared between the ranks of a multi-GPU run (ref: src/poismf.c:77-83) -----------------
// The sum over the fixed factor of half `which` (A for the B half, B for the A half) is cut into poismf_hip_session_colsum_blocks() blocks
// whose partial sums do not depend on who computes them.  A rank computes blocks [b_lo, b_hi) into the session's partial array
// (poismf_hip_session_partials: [blocks x k] real_t, device memory), receives the other blocks from its peers into the same array, and says so
// (poismf_hip_session_partials_ready): the next half-sweep then runs the fixed-order second stage only.  Same bits as the unsharded sum.
int poismf_hip_session_colsum_blocks(poismf_hip_session* s, int which) { return colsum_blocks_for(s, which ? s->dimB : s->dimA); }
int poismf_hip_session_colsum_partial(poismf_hip_session* s, int which, int b_lo, int b_hi)
{
    HIP_TRY(hipSetDevice(s->device));
    return colsum_partial(s, which ? s->dB : s->dA, which ? s->dimB : s->dimA, b_lo, b_hi);
}
real_t* poismf_hip_session_partials(poismf_hip_session* s) { return s->d_partial; }
void poismf_hip_session_partials_ready(poismf_hip_session* s) { s->partials_given = s->partials_of != nullptr; }

int poismf_hip_half_sweep(poismf_hip_session* s, int which, const poismf_hip_params* p, real_t step_size, real_t cnst_div,
                          size_t* n_unchanged)
{
    return half_sweep_impl(s, which, p, step_size, cnst_div, n_unchanged, nullptr, (real_t)0);
}

// The launches of the most recent half-sweep of half `which` ("kernel<instance> rows=N;" per launch), NUL-terminated,
// truncated to cap bytes.  Returns the untruncated length.
size_t poismf_hip_session_plan(poismf_hip_session* s, int which, char* buf, size_t cap)
{
    return copy_text(s->last_plan[which ? 1 : 0], buf, cap);
}

// Per-launch durations of half `which` since profile(1), launches of the same instance and row count added up:
// "kernel<instance> rows=R nnz=Z calls=C ms=T;" per distinct launch (T = summed milliseconds).  NUL-terminated, truncated to
// cap bytes; returns the untruncated length.
size_t poismf_hip_session_launch_profile(poismf_hip_session* s, int which, char* buf, size_t cap)
{
    (void)hipStreamSynchronize(s->stream);
    (void)hipStreamSynchronize(s->aux_stream);
    struct Agg { std::string name; unsigned rows; unsigned long long nnz; unsigned calls; double ms; };
    std::vector<Agg> agg;
    for (auto& r : s->lprof) {
        if (r.which != (which ? 1 : 0)) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.t0, r.t1) != hipSuccess) continue;
        bool found = false;
        for (auto& g : agg)
            if (g.name == r.name && g.rows == r.rows && g.nnz == r.nnz) { g.calls++; g.ms += ms; found = true; break; }
        if (!found) agg.push_back({ r.name, r.rows, r.nnz, 1u, (double)ms });
    }
    std::string t;
    for (auto& g : agg) {
        char txt[256];
        snprintf(txt, sizeof txt, "%s rows=%u nnz=%llu calls=%u ms=%.6f;", g.name.c_str(), g.rows, g.nnz, g.calls, g.ms);
        t += txt;
    }
    return copy_text(t, buf, cap);
}

int poismf_hip_half_sweep_segment(poismf_hip_session* s, int which, const poismf_hip_params* p, real_t step_size, real_t cnst_div,
                                  int seg, size_t* n_unchanged)
{
    return half_sweep_impl(s, which, p, step_size, cnst_div, n_unchanged, nullptr, (real_t)0, (real_t)1, seg);
}

}  // extern "C"
