// session.hpp -- what the host-side translation units (session.hip, planner.hip, half_sweep.hip, drivers.hip, multi_device.hip) share: the
// session object and the types it is made of, a planned launch, and the declaration of every function that crosses a unit boundary.
// Internal: the C-ABI is include/poismf_hip.h.  (struct poismf_hip_session has external linkage, so nothing here is in an anonymous namespace.)
#pragma once
#include <string>
#include <vector>

#include "plan.hpp"

constexpr size_t LDS_RESIDENT_LIMIT = 64 * 1024;  // largest tile a single wave may claim
constexpr int TEAM_LAUNCH_MAX = 32;   // team launches per pass of a half-sweep (one per team shape of a segment: seven lane-team sizes + the giant rows, or the register
                                      // teams' five shapes; half_sweep_impl refuses a plan with more)
// layout of poismf_hip_session::d_team_err, in words: [0] team launches that gave up and were re-run since the word was last read, [1] spare,
// [2 + i] set by team launch i of the current half when it gives up, [2 + TEAM_LAUNCH_MAX + i] rows launch i found unchanged (TNCG early stop:
// added to the half's counter only when the launch's results are kept)
constexpr int TEAM_ERR_WORDS = 2 + 2 * TEAM_LAUNCH_MAX;
constexpr int MAX_LAUNCHES = 256;  // launches per pass of a half-sweep that get a row-queue head: length classes are multiples of 16 up to 256, of 64
                                   // up to 2048, then powers of two (<= 60 per segment, and a pass is one segment: plan_call)

struct Bin {
    unsigned begin, count;  // range of the nnz-sorted permutation
    unsigned max_nnz;       // longest row actually in the bin (sizes tiles)
    unsigned cls;           // upper bound of the bin's length class (decides the code path: a function of the row alone)
    unsigned long long nnz; // nonzeros of the bin's rows (algorithmic bytes of a launch, bench.py's per-launch roofline)
};

struct Half {
    size_t dimM = 0, dimF = 0;
    size_t row_begin = 0, row_end = 0;  // shard
    size_t nnz = 0;
    bool x_positive = false;            // every stored value > 0 (RowParams::x_pos)
    unsigned long long* d_indptr = nullptr;
    unsigned* d_indices = nullptr;
    real_t* d_values = nullptr;
    unsigned* d_perm = nullptr;
    RowDesc* d_desc = nullptr;
    unsigned* d_eval_rows = nullptr;      // per local row: passes over its tile while profiling (allocated on demand)
    unsigned* d_dec_rows = nullptr;       // per local row: { iterations | rc << 24, evaluations } of its solver while profiling
    // The shard's rows are cut into contiguous SEGMENTS (one unless the multi-GPU driver asks for more, so that a
    // segment's rows can travel while the next one computes); within a segment rows are sorted by length and binned.
    struct Segment { unsigned row_lo, row_hi; std::vector<Bin> bins; };
    std::vector<Segment> segs;
};

struct ProfRec { hipEvent_t t0, t1; int which; };
// profiling sessions also bracket every row-bin launch (on the stream it is issued on): bench.py's per-launch roofline
struct LaunchRec { hipEvent_t t0, t1; int which; std::string name; unsigned rows; unsigned long long nnz; };

struct poismf_hip_session {
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    hipStream_t aux_stream = nullptr;  // long-row launches run here, next to the other bins
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    size_t dimA = 0, dimB = 0, k = 0;
    real_t *dA = nullptr, *dB = nullptr;
    // line-padded copies of the factors for the gathers (row stride `ld` elements = a multiple of 128 bytes), kept when
    // that cuts the bytes a gathered row drags in by >= 10 %; refreshed from the compact factor before each half-sweep
    real_t *dAp = nullptr, *dBp = nullptr;
    size_t ld = 0;
    bool padded_fresh[2] = { false, false };  // [0]: dBp mirrors dB, [1]: dAp mirrors dA
    Half half[2];  // [0]: rows of B (CSC), [1]: rows of A (CSR)
    real_t* d_bsum = nullptr;
    real_t* d_partial = nullptr;
    unsigned* d_counter = nullptr;
    unsigned* d_queue = nullptr;      // one row-queue head per launch of a half-sweep
    unsigned long long* d_team = nullptr;   // team launches (plan.hpp, TEAM_*): allocated by the first one
    unsigned long long* d_gt = nullptr;     // giant-row and lane-team launches (row_eval.hpp, GT_*): one GT_BUF_BYTES area PER LAUNCH of a half, zeroed together before the first
    size_t gt_areas = 0, team_areas = 0;    // areas d_gt / d_team hold
    unsigned* d_arrive = nullptr;           // workgroups of the forked long-row launches that have started (issue_half)
    unsigned long long gate_budget = 200000;   // ticks of the wall clock the hold-back gate waits at most: 2 ms (session_alloc)
    unsigned* d_team_err = nullptr;         // TEAM_ERR_WORDS words (above): give-ups so far, and an error word and a tally per team launch of the current half
    real_t* d_team_backup = nullptr;        // the rows the team launches of a half start from, launch after launch (restored before a re-run)
    unsigned* d_team_eval_backup = nullptr; // profiling sessions: those rows' evaluation counters (a re-run must not count an abandoned launch's evaluations)
    size_t team_backup_elems = 0, team_eval_backup_rows = 0;
    bool team_launched = false;             // since the words were last read
    bool teams_off = false;                 // a team launch of this session timed out: no more multi-CU launches for the rest of it (team_check)
    int colsum_waves = 512;           // blocks (of 8 waves) in the first stage of the column sums
    bool partials_given = false;      // d_partial already holds every block's partial sum for the NEXT half-sweep (poismf_hip_session_partials_ready)
    const real_t* partials_of = nullptr;   // ... of THIS factor (the last poismf_hip_session_colsum_partial's): a half-sweep over the other factor, a factor
                                      // written since, or a half with a caller-supplied sum does not take them for its own
    bool profiling = false;
    std::vector<ProfRec> prof;
    std::vector<LaunchRec> lprof;
    std::string last_plan[2];         // the launches of the most recent half-sweep of each half, as text
    double* d_llk = nullptr;          // scratch of poismf_hip_session_llk (allocated by its first call)
    size_t llk_cap = 0;               // ... in doubles
    void* d_topn = nullptr;           // scratch of poismf_hip_session_topn_batch and _rank_batch (allocated by its first call, grown when a call needs more)
    size_t topn_cap = 0;              // ... in bytes
    std::vector<unsigned long long> topn_indptr;   // exclude_seen: host copy of the CSR shard's row pointers (fetched by the first such call)
    int csr_rows_sorted = -1;         // exclude_seen: -1 not checked yet, 0 some resident CSR row is not strictly ascending, 1 all are
    int csc_rows_sorted = -1;         // the same of the CSC shard's rows (session_update.hip merges into ascending rows only)
    // New rows against the resident B (fold_in.hip; include/poismf_hip.h section 1m).  The rows are the A half of a GUEST: a session of its
    // own rows, factor (dA, dAp), column-sum vector, queue heads, team words and `seen` bookkeeping, which BORROWS this session's dB, dBp, ld,
    // streams and events.  Kept here from the first such call to the session's end and refilled by every later one.
    poismf_hip_session* guest = nullptr;
    bool borrows_B = false;           // set on a guest: poismf_hip_session_destroy leaves what it borrows alone
    size_t guest_rows = 0;            // on a guest: the rows its dA / dAp have room for
};

// what a half's set-up has launched and not yet collected (session.hip: finish_half_launch, finish_half_collect)
struct HalfPending { unsigned* d_len = nullptr; unsigned* d_flag = nullptr; };

// The planner's run-time knobs (testing knobs), read once per process on first use.
struct PlanKnobs {
    bool no_reg, no_team, static_rows, no_lane, no_lane_teams, no_giant_teams, no_fork, no_ls_prune;
    bool longrow_set;   // POISMF_HIP_LONGROW_NNZ was given: then it also holds for TNCG's streamed rows (plan_half)
    unsigned longrow_nnz, giant_nnz, team_spin;
};

// What plan_half decides from besides the bins: factor dimension, rows and row stride of the gathered factor; the solver as planned (POISMF_EVAL
// plans like CG), PG with one pass over each row, limit_step; poismf_hip_session::teams_off; CUs.
struct PlanCtx { size_t k, dimF, ldF; int pm; bool single_pass, limit_step, teams_off; int num_cu; };

// A launch as planned: what launch_one_here needs, plus the rows it covers and their tile geometry.  The issue loop fills in the stream,
// grid and LDS.
struct PlannedLaunch : OneLaunch {
    unsigned begin, count;      // range of the nnz-sorted permutation
    unsigned long long nnz;
    TileGeom geom;
};

// first row of segment j when a shard of nloc rows is cut into nseg segments (== dist.segment_of)
inline size_t segment_cut(size_t nloc, int j, int nseg) { return nloc * (size_t)j / (size_t)nseg; }

// planner.hip (no HIP runtime call, no launch)
std::vector<Bin> bins_of(const unsigned* len, size_t lo, size_t hi);
const PlanKnobs& plan_knobs();
size_t padded_row_bytes(size_t k);
PlanCtx plan_ctx(size_t k, size_t dimF, int method, size_t maxupd, real_t w_mult, bool limit_step, bool teams_off, int num_cu);
TileGeom long_geom(TileGeom g);
std::string launch_name(int method, const PlannedLaunch& L);
std::string plan_item(int method, const PlannedLaunch& L, bool widths = false, bool engines = false);
std::vector<std::vector<PlannedLaunch>> plan_call(const std::vector<Half::Segment>& segs, int seg, const PlanCtx& c);
size_t copy_text(const std::string& t, char* buf, size_t cap);

// session.hip
poismf_hip_session* session_alloc(int device, void* stream, size_t dimA, size_t dimB, size_t k);
int build_half(Half& h, hipStream_t stream, const real_t* val, const sparse_ix* indptr, const sparse_ix* indices,
               size_t dimM, size_t dimF, size_t r0, size_t r1, int device = 0, HalfPending* pend = nullptr);
int finish_half_collect(Half& h, hipStream_t stream, HalfPending& pend);
int finish_half(Half& h, hipStream_t stream, int nseg = 1);
int row_desc_launch(const unsigned long long* d_indptr, const unsigned* d_perm, size_t n, RowDesc* d_desc, hipStream_t stream);
void free_half(Half& h, hipStream_t stream);

// half_sweep.hip
int nc_for_k(size_t k);
int team_check(poismf_hip_session* s);
int half_sweep_impl(poismf_hip_session* s, int which, const poismf_hip_params* p, real_t step_size, real_t cnst_div,
                    size_t* n_unchanged, const real_t* bsum_override, real_t neg_step_override, real_t neg_step2 = (real_t)1,
                    int seg = -1, const Half* view = nullptr);

// drivers.hip: the interrupt flag of the running call, and its device-visible twin (nullptr until a call has allocated it)
bool interrupt_requested();
const unsigned* device_stop_word();
// drivers.hip: factors_multiple's solve (ref: src/pred.c:149-180) on a session whose A half holds the new rows and whose dA holds their start
int fold_in_solve(poismf_hip_session* s, const real_t* Bsum, real_t l2_reg, real_t w_mult, real_t step_size, size_t niter, size_t maxupd,
                  int method, bool limit_step, bool reuse_mean);

// multi_device.hip
int run_poismf_multi(const std::vector<int>& devices, real_t* A, real_t* Xr, sparse_ix* Xr_indptr, sparse_ix* Xr_indices, real_t* B, real_t* Xc,
                     sparse_ix* Xc_indptr, sparse_ix* Xc_indices, size_t dimA, size_t dimB, size_t k, const poismf_hip_params& p, size_t numiter);
std::vector<int> devices_from_env();
