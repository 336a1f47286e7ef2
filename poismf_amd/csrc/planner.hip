// planner.hip -- the planner of a half-sweep: row lengths -> length classes -> bins (bins_of), bins -> launches (plan_half: an engine and
// an instance per bin), the launches of a call (plan_call) and their names as text, the run-time knobs the plan depends on, and the
// poismf_hip_debug_plan* entry points that run all of it without a device (tests/test_plan_cpu.py).
// This unit contains no __global__ function, calls no hip* runtime function and launches nothing: keep it that way.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "session.hpp"

namespace {

// bin classes: multiples of 16 up to 256 nonzeros, multiples of 64 up to 2048 (the hand-overs between 1, 2, 4
// and 8 waves per row and between the team shapes fall on those), then powers of two.  The LDS tile of a launch is sized by the longest
// row of its bin, and LDS is what limits the waves per CU, so fine classes where most rows live buy
// occupancy (C2: 100 +- 10 nnz per row -> 7 waves per CU instead of 5).  Which ENGINE a row takes, and how
// many waves share it, is decided by the class bound alone -- never by which other rows happen to be in the
// shard -- so a row's arithmetic does not depend on how the matrix is cut into shards.
unsigned length_class(unsigned n)
{
    if (n <= 256) return std::max(16u, (n + 15u) / 16u * 16u);
    if (n <= 2048) return (n + 63u) / 64u * 64u;   // (up to the longest team row: every class maps to ONE team shape, plan.hpp team_shape_for)
    unsigned cls = 4096;
    while (cls < n) cls <<= 1;
    return cls;
}

bool prefetch_enabled() { return true; }   // (streamed rows request the next chunk's tile a chunk ahead: row_eval.hpp, PF)

TileGeom plan_geom(size_t k, unsigned bin_max_nnz, bool single_pass, bool want_pq)
{
    TileGeom g;
    g.k = (int)k;
    g.pq_cap = 0;
    g.prefetch = 0;
    g.zero_row = 0;
    g.ldF = (int)k;
    g.s_load = (int)((k * sizeof(real_t) + 15) / 16);
    g.s_stride = g.s_load | 1;
    g.group = g.s_load <= 16 ? 16 : (g.s_load <= 32 ? 32 : 64);
    // tile capacity: whole rows of this bin if that fits the per-wave budget, else stream in chunks.
    // A single-pass solver (PG with one update) gains nothing from residency: keep tiles small there
    // so that many waves per CU keep gathers in flight.
    const unsigned want = std::max(16u, bin_max_nnz);
    // chunk for streamed rows: ~14 KiB of tile per wave keeps >= 10 waves per CU gathering (measured on C2:
    // 128-nonzero chunks 1.46 ms per sweep, 64 or 32: 0.80-0.85 ms)
    unsigned stream_chunk = (unsigned)(14336 / ((size_t)g.s_stride * 16)) / 16 * 16;
    stream_chunk = std::min(128u, std::max(16u, stream_chunk));
    // multi-pass solvers: at least 32 nonzeros per chunk while four such tiles still fit a CU's LDS next to everything
    // else (C5, TNCG fp64 k = 100: 16 -> 32 nonzeros takes the B half from 1091 to 956 ms; 48: 1051)
    if (!single_pass && (size_t)32 * g.s_stride * 16 <= 28 * 1024) stream_chunk = std::max(stream_chunk, 32u);
    // with the next chunk's tile requested a chunk ahead (row_eval.hpp, PF) a larger chunk amortises the per-chunk
    // overhead without exposing its gather: as many nonzeros as the PMF_PRE slots per lane in flight hold
    // (C3 B half, CG fp64: 32 nonzeros without prefetch 103.9 ms, with 96.6; 48 with prefetch 82.6; 64 without 111.7)
    if (!single_pass && prefetch_enabled() && ((size_t)g.s_load == (size_t)SPECIAL_SL_A || (size_t)g.s_load == (size_t)SPECIAL_SL_B))
        stream_chunk = std::max(stream_chunk, std::max(16u, (unsigned)(PMF_PRE * WAVE / g.s_load) / 16 * 16));
    unsigned cap = want;
    g.resident = 1;
    TileGeom probe = g;
    probe.cap = (int)cap;
    if (lds_bytes_per_wave(probe, sizeof(real_t)) > LDS_RESIDENT_LIMIT || (single_pass && cap > stream_chunk)) {
        cap = stream_chunk;
        probe.cap = (int)cap;
        while (cap > 16 && lds_bytes_per_wave(probe, sizeof(real_t)) > LDS_RESIDENT_LIMIT) { cap /= 2; probe.cap = (int)cap; }
        g.resident = 0;
    }
    g.cap = (int)cap;
    // CG: cache T.x and T.d per nonzero when both fit next to the tile (up to 48 KiB for the pair); longer rows
    // fall back to the direct line search
    // Only for streamed rows: there every line-search trial would otherwise be a fresh gather from L2/HBM
    // (C3 B half: 247 -> 146 ms).  For LDS-resident rows a trial is a cheap pass over the tile already and the
    // cached variant buys nothing: it halves the passes over the tile (C2 CG fp64: 20 -> 10 per row) and the sweep takes
    // the same 10.3 ms -- those rows are bound by the solver's chain of k-vector reductions and scalar decisions at one
    // wave per SIMD, not by the tile passes.
    if (want_pq && !g.resident && (size_t)2 * bin_max_nnz * sizeof(real_t) <= 48 * 1024)
        g.pq_cap = (int)((bin_max_nnz + 15u) / 16u * 16u);
    g.prefetch = (!g.resident && prefetch_enabled()) ? 1 : 0;
    return g;
}

// poismf_hip_debug_lane_full_width (testing aid): != 0 -- the lane launches planned from now on carry every element of their slots, also where an
// instance specialised on the used width exists (plan.hpp, lane_used_width): the two must agree bit for bit (tests/test_gpu_lane_width.py)
std::atomic<int> g_lane_full_width{0};
// poismf_hip_debug_reg_quad_off (testing aid): != 0 -- the one-wave register launches planned from now on take the sixteen-lane engine also where
// the quad engine exists (plan.hpp, reg_quad): one process can run both (tests/test_gpu_quad.py)
std::atomic<int> g_reg_quad_off{0};

}  // namespace

// The length bins of one segment: len[lo .. hi) are its rows' lengths, sorted (longest first).
std::vector<Bin> bins_of(const unsigned* len, size_t lo, size_t hi)
{
    std::vector<Bin> bins;
    for (size_t i = lo; i < hi; i++) {
        const unsigned cls = length_class(len[i]);
        if (bins.empty() || cls != bins.back().cls) bins.push_back({ (unsigned)i, 0u, len[i], cls, 0ull });   // sorted: the first row of a bin is its longest
        bins.back().count++;
        bins.back().nnz += len[i];
    }
    return bins;
}

// The planner's run-time knobs (testing knobs), read once per process on first use.
const PlanKnobs& plan_knobs()
{
    static const PlanKnobs kn = [] {
        PlanKnobs k{};
        k.no_reg = getenv("POISMF_HIP_NO_REGTILE") != nullptr;   // (the LDS engine for every row)
        k.no_team = getenv("POISMF_HIP_NO_TEAM") != nullptr; k.static_rows = getenv("POISMF_HIP_STATIC_ROWS") != nullptr;
        k.no_lane = getenv("POISMF_HIP_NO_LANE") != nullptr; k.no_lane_teams = getenv("POISMF_HIP_NO_LANE_TEAMS") != nullptr;
        k.no_giant_teams = getenv("POISMF_HIP_NO_GIANT_TEAMS") != nullptr; k.no_fork = getenv("POISMF_HIP_NO_FORK") != nullptr;
        k.no_ls_prune = getenv("POISMF_HIP_NO_LS_PRUNE") != nullptr;   // (evaluate every line-search trial)
        const char* e = getenv("POISMF_HIP_LONGROW_NNZ");             // (a huge value: no eight-wave rows at all)
        k.longrow_set = e != nullptr;
        k.longrow_nnz = e != nullptr ? (unsigned)std::max(64, atoi(e)) : LONG_ROW_NNZ;
        e = getenv("POISMF_HIP_GIANT_NNZ");
        k.giant_nnz = e != nullptr ? (unsigned)std::max(64, atoi(e)) : LONG_ROW_NNZ;
        e = getenv("POISMF_HIP_TEAM_SPIN_LIMIT");
        k.team_spin = e != nullptr ? (unsigned)std::max(1, atoi(e)) : TEAM_SPIN_LIMIT;
        return k;
    }();
    return kn;
}

// Bytes of a factor row of k elements in the line-padded gather copies (== k * sizeof(real_t): the session keeps no such copy).
size_t padded_row_bytes(size_t k)
{
    const size_t rowb = k * sizeof(real_t);
    size_t padb = (rowb + 127) / 128 * 128;
    static const bool no_pad = getenv("POISMF_HIP_NO_PAD") != nullptr;  // testing knob
    const bool line_pad = !no_pad && padb != rowb && (double)padb <= 0.9 * (double)(rowb + 120);
    // and a row that does not end on a 16-byte slot boundary is padded to one in any case: the gathers fetch whole
    // slots and rely on the excess of the last one being zero
    if (!line_pad) padb = (rowb + 15) / 16 * 16;
    return padb;
}

PlanCtx plan_ctx(size_t k, size_t dimF, int method, size_t maxupd, real_t w_mult, bool limit_step, bool teams_off, int num_cu)
{
    const int pm = plan_method(method);   // the evaluation-only kernels (plan.hpp, K_EVAL) are planned like CG
    const bool single_pass = method == POISMF_PG && maxupd <= 1 && w_mult == (real_t)1.;
    return { k, dimF, padded_row_bytes(k) / sizeof(real_t), pm, single_pass, limit_step, teams_off, num_cu };
}

// The eight-wave streamed kernel's geometry for rows of geometry g: every wave streams its own chunks, sized so that LONG_NW
// private tiles and the reduction scratch fit in one CU's LDS.
TileGeom long_geom(TileGeom g)
{
    g.resident = 0; g.prefetch = prefetch_enabled() ? 1 : 0; g.pq_cap = 0;
    for (int cap = 128;; cap -= 16) {
        g.cap = cap;
        if (cap <= 16 || lds_bytes_per_block(g, sizeof(real_t), LONG_NW) <= 150 * 1024) break;
    }
    return g;
}

namespace {

// Row bins -> launches: an engine and an instance per bin; consecutive bins that can share an instance share a launch.
std::vector<PlannedLaunch> plan_half(const std::vector<Bin>& bins, const PlanCtx& c)
{
    const PlanKnobs& kn = plan_knobs();
    const int pm = c.pm;
    std::vector<PlannedLaunch> launches;
    // The bin joins the previous launch if that launch has the same engine, ends where the bin begins and joins(previous) holds; else it opens one.
    auto place = [&](const Bin& b, Engine e, const TileGeom& g, int nw, int S, int team, const LaneShape& lane, auto joins) {
        if (!launches.empty() && launches.back().engine == e && launches.back().begin + launches.back().count == b.begin && joins(launches.back()))
            { launches.back().count += b.count; launches.back().nnz += b.nnz; return; }
        PlannedLaunch L{};
        L.engine = e; L.nw = nw; L.reg_S = S; L.team = team; L.lane = lane; L.s_load = g.s_load; L.spl = slots_per_lane(c.k);
        L.begin = b.begin; L.count = b.count; L.nnz = b.nnz; L.geom = g; L.geom.zero_row = (unsigned)c.dimF; L.geom.ldF = (int)c.ldF;
        launches.push_back(L);
    };
    // register engine: factor rows of at most 16 slots (32 for doubles, two slots per lane), and 24-bit row ids / 32-bit
    // byte offsets into the factor
    const int reg_ns = reg_slots_per_lane((c.k * sizeof(real_t) + 15) / 16);
    const bool reg_ok = !kn.no_reg && reg_ns > 0 &&
                        c.dimF < ((size_t)1 << 24) && (c.dimF + 1) * c.ldF * sizeof(real_t) + 16 < ((size_t)1 << 32);
    // two slots per lane: single-wave rows only, and shorter ones for CG and TNCG (plan.hpp, REG2_NNZ_MAX_*)
    const bool regw_ok = reg_ok && (reg_ns == 1 || REG_G == 8);
    const unsigned reg_max = reg_nnz_max(pm, reg_ns);
    // (a bin of a few thousand rows is not worth a launch of its own: it rides along with the next longer size.  TNC keeps the tile size its
    // length class names: in fp32 its results move in the last bits with the size of the instance -- 62 of 900 rows in tests/test_gpu_parity.py's
    // segment test -- and a row must not depend on which other rows share its shard; PG and CG, and fp64 TNC, are bit-identical across instances)
    const bool ride = pm != POISMF_TNCG || sizeof(real_t) == 8;
    // teams: CG on doubles with two slots per lane (k = 50 fp64: 25 slots), rows handed out through the queue
    const bool no_team = kn.no_team || c.teams_off;
    const bool team_ok = !no_team && !kn.static_rows && reg_ok && reg_ns == 2 && REG_G == 16 && sizeof(real_t) == 8 && pm == POISMF_CG;
    // lane-per-nonzero engine (lane_eval.hpp): 24-bit row ids and row strides, 32-bit byte offsets into the factor (as the register engine)
    const bool lane_ok = !kn.no_lane && !c.single_pass && c.dimF < ((size_t)1 << 24) && c.ldF * sizeof(real_t) < ((size_t)1 << 24) &&
                         (c.dimF + 1) * c.ldF * sizeof(real_t) + 16 < ((size_t)1 << 32);
    const bool no_long = kn.longrow_nnz >= 0x40000000u;
    for (const Bin& b : bins) {
        TileGeom g = plan_geom(c.k, b.cls, c.single_pass, pm == POISMF_CG && c.limit_step);
        if (c.single_pass) { g.resident = 0; g.prefetch = prefetch_enabled() ? 1 : 0; }  // one pass: "gather once" and "stream" are the same thing
        if (lane_ok) {
            LaneShape ls = lane_shape_for(b.cls, g.s_load, pm);
            if (ls.waves > 0 && g_lane_full_width.load(std::memory_order_relaxed) == 0) ls.ku = lane_used_width(c.k, g.s_load, pm, ls);
            // k = 100 fp64 rows above 64 nonzeros on the B half: rounds 3-4 left them to the streamed launch (with only the 65 .. 128-nonzero rows
            // taken out, that launch lost the short-row tail that kept its wave slots busy: B half 234.6 -> 296.0 ms); since round 5 every row up
            // to 384 nonzeros has a resident instance and the streamed launch keeps the 3 k rows above.
            // k = 100 fp64 under TNCG, rows of 385 .. 8192 nonzeros (round 5): a TEAM of ceil(class / 384) four-wave workgroups keeps the row
            // RESIDENT (each member its 1/M of the nonzeros in one register set + a partial LDS set per wave, lane_eval.hpp TM_) and the members
            // exchange their sums per evaluation -- instead of re-streaming 800 bytes per nonzero for each of ~70 evaluations (84 % of config C5's
            // 697 GB per sweep).  The team size is a function of the row's length class alone.  POISMF_HIP_NO_LANE_TEAMS=1: the eight-wave
            // streamed kernel (round 5a)
            int lane_team = 0;
            if (ls.waves == 0 && sizeof(real_t) == 8 && g.s_load == LANE_TEAM_KS && pm == POISMF_TNCG && !kn.no_lane_teams && !no_team && !kn.static_rows &&
                b.cls > LANE_TEAM_NNZ && b.cls <= LONG_ROW_NNZ) {
                const int m = (int)((b.cls + LANE_TEAM_NNZ - 1u) / LANE_TEAM_NNZ);
                if (m >= 2 && c.num_cu >= 2 * m) { ls = LANE_TEAM_SHAPE; lane_team = m; }
            }
            if (ls.waves > 0) {
                place(b, lane_team ? Engine::LaneTeam : Engine::Lane, g, ls.waves, 0, lane_team, ls,
                      [&](const PlannedLaunch& P) { return P.team == lane_team && P.lane == ls; });
                continue;
            }
        }
        if (reg_ok && b.cls <= reg_max) {
            // short rows: the tile lives in registers (reg_eval.hpp); bins sharing a step count share a launch
            const int S = reg_steps_for(ride ? b.max_nnz : b.cls);
            place(b, Engine::Reg, g, 1, S, 0, LaneShape{},
                  [&](const PlannedLaunch& P) { return P.reg_S >= S && (P.reg_S == S || (ride && b.count < 4096u)); });
            // (one decision per plan: every Reg launch of it gets the same answer, so joining bins never mixes the two engines)
            launches.back().quad = g_reg_quad_off.load(std::memory_order_relaxed) == 0 ? reg_quad(c.k, g.s_load, pm, c.ldF) : 0;
            continue;
        }
        if (regw_ok && b.cls <= regw_nnz_max(pm)) {
            // medium rows: 2, 4 or 8 waves share a row, each keeps its part of the tile in registers
            const int nw = regw_waves_for(b.cls, pm);
            const int S = regw_steps_for(ride ? b.max_nnz : b.cls, nw);
            place(b, Engine::RegW, g, nw, S, 0, LaneShape{},
                  [&](const PlannedLaunch& P) { return P.nw == nw && P.reg_S >= S && (P.reg_S == S || (ride && b.count < 2048u)); });
            continue;
        }
        if (team_ok) {
            // rows whose tile fits the registers of two to four CUs, not of one: a team per row (reg_eval.hpp, M_ > 1) -- by the class bound,
            // never by the longest row that happens to be in the bin: a row's share of the tile (my_share: C = ceil(nnz / (NW M))) -- and with it
            // its summation order -- must not depend on its shard
            const TeamShape ts = team_shape_for(b.cls);
            if (ts.members > 0) {
                place(b, Engine::RegTeam, g, TEAM_NW, ts.steps, ts.members, LaneShape{},
                      [&](const PlannedLaunch& P) { return P.team == ts.members && P.reg_S == ts.steps; });
                continue;
            }
        }
        // TNCG streams a non-resident row once per evaluation (~70 of them): one wave keeps ~8 KB of gathers in flight (~4 GB/s), and once
        // the lane engine holds every row up to 384 nonzeros the few thousand longer ones are a tail, not a crowd -- config C5, rows of
        // 385 .. 8192 nonzeros on one wave each: 229 ms; on eight-wave workgroups: inside the 133 ms of the then-giant-row-bound launch.
        // So TNCG's streamed rows always take the eight-wave kernel (POISMF_HIP_LONGROW_NNZ overrides; CG caches its line search, PG
        // makes one gather per pass over the whole chip: they keep the one-wave streamed kernel below 8192 nonzeros).
        const unsigned long_thr_here = (pm == POISMF_TNCG && !g.resident && !kn.longrow_set) ? 0u : kn.longrow_nnz;
        const TileGeom gl = long_geom(g);
        // (round 6: eight private tiles of even 16 nonzeros do not fit a CU's LDS once a factor row is ~1.2 KB -- k > 146 in fp64, > 292 in fp32 --
        // and the launch failed with "invalid argument", i.e. rc 1 for a TNCG fit at k = 200 fp64 with any row past the resident limit, found by
        // scripts/knob_matrix.sh under POISMF_HIP_LONGROW_NNZ=256: such rows keep the one-wave streamed kernel below)
        const bool long_fits = lds_bytes_per_block(gl, sizeof(real_t), LONG_NW) <= LDS_PER_CU;
        if (!no_long && long_fits && b.cls > long_thr_here) {
            // TNCG re-streams such a row for every evaluation: a team of GT_M workgroups per row (row_eval.hpp, TM; POISMF_HIP_NO_GIANT_TEAMS=1:
            // one workgroup per row, rounds 1-4).  Decided by the solver alone: a row's arithmetic must not depend on its shard.
            const bool giant = !kn.no_giant_teams && !no_team && !kn.static_rows && pm == POISMF_TNCG && b.cls > kn.giant_nnz && c.num_cu >= 2 * GT_M;
            place(b, giant ? Engine::Giant : Engine::LdsLong, gl, LONG_NW, 0, giant ? GT_M : 0, LaneShape{}, [](const PlannedLaunch&) { return true; });
            continue;
        }
        place(b, Engine::Lds, g, 1, 0, 0, LaneShape{}, [&](const PlannedLaunch& P) {
            return g.resident == 0 && P.geom.resident == 0 && g.pq_cap == 0 && P.geom.pq_cap == 0 && P.geom.cap == g.cap;
        });
    }
    return launches;
}

}  // namespace

// The kernel instance a launch runs, as plan() and the launch profile name it.
std::string launch_name(int method, const PlannedLaunch& L)
{
    const char* m = method == POISMF_PG ? "pg" : method == POISMF_EVAL ? "eval" : method == POISMF_CG ? "cg" : "tncg";
    const char* t = sizeof(real_t) == 4 ? "float" : "double";
    const LaneShape& l = L.lane;
    char txt[160] = "", lp[16] = "";
    if (l.lp != 0) snprintf(lp, sizeof lp, "+%d", l.lp);
    switch (L.engine) {
        case Engine::LaneTeam: snprintf(txt, sizeof txt, "half_sweep_lane_team_kernel<%s,%s,KS=%d,V=%d,L=0+%d,NW=%d,M=%d>", t, m, L.geom.s_load, l.lv, l.lp, L.nw, L.team); break;
        case Engine::Lane:
            snprintf(txt, sizeof txt, "half_sweep_lane_kernel<%s,%s,KS=%d,V=%d,A=%d,L=%d%s,NW=%d%s%s>", t, m, L.geom.s_load, l.lv, l.la, l.ll,
                     lp, L.nw, l.small ? ",2/SIMD" : "", l.tx == 48 ? ",TX=48" : l.tx == 64 ? ",TX=64" : "");
            break;
        case Engine::Giant: snprintf(txt, sizeof txt, "half_sweep_giant_kernel<%s,%s,NW=%d,M=%d,streamed cap=%d>", t, m, L.nw, L.team, L.geom.cap); break;
        case Engine::RegTeam: snprintf(txt, sizeof txt, "half_sweep_team_kernel<%s,%s,S=%d,NW=%d,M=%d>", t, m, L.reg_S, L.nw, L.team); break;
        case Engine::Reg: snprintf(txt, sizeof txt, "half_sweep_reg_kernel<%s,%s,S=%d>", t, m, L.reg_S); break;
        case Engine::RegW: snprintf(txt, sizeof txt, "half_sweep_regw_kernel<%s,%s,S=%d,NW=%d>", t, m, L.reg_S, L.nw); break;
        case Engine::Lds:
        case Engine::LdsLong:
            snprintf(txt, sizeof txt, "half_sweep_kernel<%s,%s,NW=%d,%s cap=%d>", t, m, L.nw, L.geom.resident ? "resident" : "streamed", L.geom.cap);
            break;
    }
    return txt;
}

// ... and as poismf_hip_session_plan lists it (widths: a lane launch specialised on the used width says so behind its name, "...>[KU=50]" --
// poismf_hip_debug_plan_widths; engines: a one-wave register launch on the quad engine says so too, "...>[quad]" -- poismf_hip_debug_plan_engines;
// the names themselves are what they were before such instances existed)
std::string plan_item(int method, const PlannedLaunch& L, bool widths, bool engines)
{
    std::string name = launch_name(method, L);
    if (widths && L.engine == Engine::Lane && L.lane.ku > 0) name += "[KU=" + std::to_string(L.lane.ku) + "]";
    if (engines && L.engine == Engine::Reg && L.quad != 0) name += "[quad]";
    return name + " rows=" + std::to_string(L.count) + ";";
}

// The launches of one half-sweep call over segment `seg` of a half, or (seg < 0) over all of its segments, as the passes the call makes: one
// per segment, each planned from that segment's bins alone and run as a call over that segment would run it.  So a row's launch -- its engine,
// instance and team -- does not depend on which segments a call names, and the per-launch resources (row-queue heads, team areas and words)
// are a segment's however many segments there are.
std::vector<std::vector<PlannedLaunch>> plan_call(const std::vector<Half::Segment>& segs, int seg, const PlanCtx& c)
{
    std::vector<std::vector<PlannedLaunch>> passes;
    for (size_t j = 0; j < segs.size(); j++)
        if (seg < 0 || (size_t)seg == j) passes.push_back(plan_half(segs[j].bins, c));
    if (passes.empty()) passes.emplace_back();   // (a half without segments: the prologue and the epilogue run all the same)
    return passes;
}

// a text report into the caller's buffer: NUL-terminated, truncated to cap bytes; returns the untruncated length
size_t copy_text(const std::string& t, char* buf, size_t cap)
{
    if (cap > 0) {
        const size_t n = std::min(cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return t.size();
}

// Whether the solver's row-kernel translation unit has the instance launch L names: the dispatcher's own answer, from a dry run of the launch
// (plan.hpp, OneLaunch::dry -- no HIP call).
static bool has_instance(int method, const PlannedLaunch& L)
{
    OneLaunch o = L;
    o.dry = 1;
    HalfArgs<real_t> a{};
    a.nrows = L.count; a.geom = L.geom;
    return pmf_launch_one(method, o, a) == 0;
}

// Testing aid: the planner without a device.  Rows of row_nnz[0 .. nrows) nonzeros, cut into nseg segments, sorted and binned as
// finish_half_launch / finish_half_collect do it; then the plan of a half-sweep call over segment `seg` (< 0: over all of them), as
// poismf_hip_session_plan words it.  No HIP call.
static size_t debug_plan_impl(const unsigned* row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method, size_t maxupd,
                              real_t w_mult, int limit_step, int num_cu, char* buf, size_t cap, bool widths, bool engines = false, bool missing = false)
{
    std::string text;
    nseg = std::max(nseg, 1);
    if (k > 0 && slots_per_lane(k) != 0 && seg < nseg) {
        std::vector<unsigned> len(row_nnz, row_nnz + nrows);
        std::vector<Half::Segment> segs;
        for (int j = 0; j < nseg; j++) {
            const size_t lo = segment_cut(nrows, j, nseg), hi = segment_cut(nrows, j + 1, nseg);
            std::stable_sort(len.begin() + lo, len.begin() + hi, std::greater<unsigned>());
            segs.push_back({ (unsigned)lo, (unsigned)hi, bins_of(len.data(), lo, hi) });
        }
        const PlanCtx c = plan_ctx(k, dimF, method, maxupd, w_mult, limit_step != 0, false, num_cu);
        for (const auto& pass : plan_call(segs, seg, c))
            for (const PlannedLaunch& L : pass)
                if (!missing || !has_instance(method, L)) text += plan_item(method, L, widths, engines);
    }
    return copy_text(text, buf, cap);
}

extern "C" {

size_t poismf_hip_debug_plan(const unsigned* row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method, size_t maxupd,
                             real_t w_mult, int limit_step, int num_cu, char* buf, size_t cap)
{
    return debug_plan_impl(row_nnz, nrows, nseg, seg, k, dimF, method, maxupd, w_mult, limit_step, num_cu, buf, cap, false);
}
// The same plan, every lane launch that is specialised on the used width of its factor rows marked "[KU=<width>]" behind its name.
size_t poismf_hip_debug_plan_widths(const unsigned* row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method, size_t maxupd,
                                    real_t w_mult, int limit_step, int num_cu, char* buf, size_t cap)
{
    return debug_plan_impl(row_nnz, nrows, nseg, seg, k, dimF, method, maxupd, w_mult, limit_step, num_cu, buf, cap, true);
}
// The listing of poismf_hip_debug_plan_widths, every one-wave register launch that takes the quad engine (plan.hpp, reg_quad) marked "[quad]" as well.
size_t poismf_hip_debug_plan_engines(const unsigned* row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method, size_t maxupd,
                                     real_t w_mult, int limit_step, int num_cu, char* buf, size_t cap)
{
    return debug_plan_impl(row_nnz, nrows, nseg, seg, k, dimF, method, maxupd, w_mult, limit_step, num_cu, buf, cap, true, true);
}
// Of that listing, the launches for which the solver's translation unit has no kernel instance (poismf_hip.hip, launch_one_here): nothing, unless
// the planner names something the dispatcher lacks.
size_t poismf_hip_debug_plan_missing(const unsigned* row_nnz, size_t nrows, int nseg, int seg, size_t k, size_t dimF, int method, size_t maxupd,
                                     real_t w_mult, int limit_step, int num_cu, char* buf, size_t cap)
{
    return debug_plan_impl(row_nnz, nrows, nseg, seg, k, dimF, method, maxupd, w_mult, limit_step, num_cu, buf, cap, true, true, true);
}
// Testing aid: != 0 -- from now on this process plans its lane launches on the instances that carry every element of their slots (what a
// -DPMF_LANE_KU50=0 build always does); 0 -- the default again.  Returns the previous setting.
int poismf_hip_debug_lane_full_width(int full) { return g_lane_full_width.exchange(full != 0 ? 1 : 0); }
// Testing aid: != 0 -- from now on this process plans its one-wave register launches on the sixteen-lane engine (what a -DPMF_REG_QUAD=0 build
// always does); 0 -- the default again.  Returns the previous setting.
int poismf_hip_debug_reg_quad_off(int off) { return g_reg_quad_off.exchange(off != 0 ? 1 : 0); }

}  // extern "C"
