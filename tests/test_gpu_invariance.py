"""A row's result never depends on the rows it is planned with -- in bits, on the device.

One ragged A-side problem per case: a row per length class (bounds 16 .. 256 by 16, 320 .. 2048 by 64, then 3000, 5000, 9000 and 20000 nonzeros)
plus a row just above every engine hand-over, that list once per segment (NREP times), so every segment of a cut holds every class.  Only the
A half runs, from set_factors(A0, B0): a row then depends on its own nonzeros, on B and on B's column sums, which no variant changes.  The
baseline is one session, one segment, one call; every variant must give EVERY row the same bits:

  a  segments one by one, 2 and 8 of them                  d  the rows in reverse order (compared under the permutation)
  b  8 (and 5) segments in ONE call                         e  7500 filler rows in two register classes added (plan_half's `ride` thresholds)
  c  three sharded sessions with uneven cuts                f  run_poismf over the device list 0,0,0 against one device (child processes)

Equal bits between wrong answers prove nothing: every case's baseline is also judged against the checker's A half by the rules of
tests/test_gpu_parity.py / test_gpu_regtile.py / test_gpu_regpair.py / test_gpu_giant.py, tolerances unchanged.  The plan of every case must name the engines listed for it (tests/test_plan_cpu.py holds the lists
to the planner, and to every engine and instance shape reachable at the case's k, without a device).  Needs an MI355X."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from poismf_amd import api, harness
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLASS_BOUNDS = list(range(16, 257, 16)) + list(range(320, 2049, 64)) + [3000, 5000, 9000, 20000]     # 48 rows, 72 328 nonzeros
HAND_OVERS = [c + 1 for c in (48, 64, 96, 112, 128, 144, 160, 192, 256, 288, 320, 384, 512, 576, 640, 768, 1024, 1088, 1152, 1280, 1536,
                              2048, 4096, 8192)]
SEGMENT_LENGTHS = CLASS_BOUNDS + HAND_OVERS
NREP = 8
DIMB = 24000

# case -> (solver, floats, k, maxupd, what the A half's plan must name).  Read off the planner (tests/test_plan_cpu.py checks them against it)
CASES = {
    "tncg-f64-k100": ("tncg", False, 100, 10, ["lane_kernel<double,tncg,KS=50,V=1,A=0,L=0,NW=1,TX=48>", "lane_kernel<double,tncg,KS=50,V=1,A=0,L=0,NW=1,TX=64>",
                                               "lane_kernel<double,tncg,KS=50,V=1,A=0,L=0,NW=2>", "lane_kernel<double,tncg,KS=50,V=1,A=0,L=0+32,NW=4>"] +
                      [f"lane_team_kernel<double,tncg,KS=50,V=1,L=0+32,NW=4,M={m}>" for m in (2, 3, 4, 5, 6, 11, 22)] + ["giant_kernel<double,tncg,NW=8,M=32"]),
    "cg-f64-k50": ("cg", False, 50, 5, ["lane_kernel<double,cg,KS=25,V=1,A=0,L=0,NW=1,2/SIMD>", "lane_kernel<double,cg,KS=25,V=1,A=0,L=0+32,NW=1,2/SIMD>",
                                        "lane_kernel<double,cg,KS=25,V=1,A=0,L=1,NW=1>", "lane_kernel<double,cg,KS=25,V=1,A=2,L=1,NW=1>",
                                        "lane_kernel<double,cg,KS=25,V=1,A=2,L=1,NW=2>", "lane_kernel<double,cg,KS=25,V=1,A=2,L=1,NW=4>",
                                        "lane_kernel<double,cg,KS=25,V=1,A=2,L=1+16,NW=4>", "team_kernel<double,cg,S=36,NW=4,M=2>", "team_kernel<double,cg,S=28,NW=4,M=3>",
                                        "team_kernel<double,cg,S=32,NW=4,M=3>", "team_kernel<double,cg,S=32,NW=4,M=4>", "kernel<double,cg,NW=1,streamed", "kernel<double,cg,NW=8,streamed"]),
    "tncg-f64-k50": ("tncg", False, 50, 10, ["lane_kernel<double,tncg,KS=25,V=1,A=0,L=0,NW=1,2/SIMD>", "lane_kernel<double,tncg,KS=25,V=1,A=0,L=1,NW=1>",
                                             "lane_kernel<double,tncg,KS=25,V=1,A=2,L=1,NW=1>", "lane_kernel<double,tncg,KS=25,V=1,A=2,L=1,NW=2>",
                                             "lane_kernel<double,tncg,KS=25,V=1,A=2,L=1,NW=4>", "lane_kernel<double,tncg,KS=25,V=1,A=2,L=1+16,NW=4>",
                                             "kernel<double,tncg,NW=8,streamed", "giant_kernel<double,tncg,NW=8,M=32"]),
    "pg-f32-k50": ("pg", True, 50, 10, ["reg_kernel<float,pg,S=", "regw_kernel<float,pg,S=40,NW=2>", "regw_kernel<float,pg,S=32,NW=4>", "regw_kernel<float,pg,S=40,NW=8>",
                                        "lane_kernel<float,pg,KS=13,V=4,A=0,L=0,NW=4,2/SIMD>", "lane_kernel<float,pg,KS=13,V=4,A=0,L=0+16,NW=4,2/SIMD>",
                                        "kernel<float,pg,NW=1,streamed", "kernel<float,pg,NW=8,streamed"]),
    "pg-f32-k50-single-pass": ("pg", True, 50, 1, ["reg_kernel<float,pg,S=", "regw_kernel<float,pg,S=40,NW=2>", "regw_kernel<float,pg,S=40,NW=4>", "regw_kernel<float,pg,S=40,NW=8>",
                                                   "kernel<float,pg,NW=1,streamed", "kernel<float,pg,NW=8,streamed"]),
    "cg-f32-k50": ("cg", True, 50, 5, [f"lane_kernel<float,cg,KS=13,V={v},A=0,L=0,NW={nw},2/SIMD>" for v, nw in ((1, 1), (2, 1), (2, 2), (2, 4), (2, 8), (3, 8))] +
                   ["kernel<float,cg,NW=1,streamed", "kernel<float,cg,NW=8,streamed"]),
    "tncg-f32-k50": ("tncg", True, 50, 10, [f"lane_kernel<float,tncg,KS=13,V={v},A=0,L=0,NW={nw},2/SIMD>" for v, nw in ((1, 1), (2, 1), (2, 2), (2, 4), (2, 8), (3, 8))] +
                     ["kernel<float,tncg,NW=8,streamed", "giant_kernel<float,tncg,NW=8,M=32"]),
    "pg-f64-k50": ("pg", False, 50, 10, ["reg_kernel<double,pg,S=", "kernel<double,pg,NW=1,streamed", "kernel<double,pg,NW=8,streamed"]),
    "cg-f64-k20": ("cg", False, 20, 5, ["reg_kernel<double,cg,S=", "regw_kernel<double,cg,S=32,NW=2>", "regw_kernel<double,cg,S=36,NW=4>", "regw_kernel<double,cg,S=36,NW=8>",
                                        "kernel<double,cg,NW=1,streamed", "kernel<double,cg,NW=8,streamed"]),
    "tncg-f32-k20": ("tncg", True, 20, 10, [f"reg_kernel<float,tncg,S={s}>" for s in range(4, 41, 4)] + ["regw_kernel<float,tncg,S=24,NW=2>", "regw_kernel<float,tncg,S=16,NW=4>",
                                            "regw_kernel<float,tncg,S=24,NW=8>", "kernel<float,tncg,NW=8,streamed", "giant_kernel<float,tncg,NW=8,M=32"]),
    "pg-f32-k7": ("pg", True, 7, 10, ["reg_kernel<float,pg,S=", "regw_kernel<float,pg,S=40,NW=2>", "regw_kernel<float,pg,S=40,NW=4>", "regw_kernel<float,pg,S=40,NW=8>",
                                      "kernel<float,pg,NW=1,streamed", "kernel<float,pg,NW=8,streamed"]),
    "cg-f64-k33": ("cg", False, 33, 5, ["reg_kernel<double,cg,S=", "kernel<double,cg,NW=1,resident", "team_kernel<double,cg,S=32,NW=4,M=2>", "team_kernel<double,cg,S=36,NW=4,M=2>",
                                        "team_kernel<double,cg,S=28,NW=4,M=3>", "team_kernel<double,cg,S=32,NW=4,M=3>", "team_kernel<double,cg,S=32,NW=4,M=4>",
                                        "kernel<double,cg,NW=1,streamed", "kernel<double,cg,NW=8,streamed"]),
}
KNOBS_SET = [v for v in os.environ if v.startswith("POISMF_HIP_")]   # under a testing knob the plan may lack a path: bits are compared all the same


def case_lengths(nrep=NREP):
    return SEGMENT_LENGTHS * nrep


def problem(case, lengths=None, seed=41):
    from tests.test_gpu_regtile import ragged_problem
    method, prec, k, maxupd, _ = CASES[case]
    return ragged_problem(case_lengths() if lengths is None else lengths, DIMB, k, prec, seed=seed)


def params_for(s, case):
    method, prec, k, maxupd, _ = CASES[case]
    l2, _, _ = harness.auto_defaults(method, k)
    kw = dict(early_stop=True) if method == "tncg" else {}
    return s.make_params(method, l2, maxupd=maxupd, **kw), s.cnst_div(l2, 1e-7)


def a_half(s, case, A0, B0, segs=None):
    """the A half from (A0, B0): in one call (segs None) or segment by segment; returns (A, rows TNCG left unchanged)"""
    method = CASES[case][0]
    p, cd = params_for(s, case)
    s.set_factors(A0, B0)
    if segs is None:
        n = s.half_sweep(1, p, 1e-7, cd, want_unchanged=method == "tncg")
    else:
        for j in range(segs):
            n = s.half_sweep(1, p, 1e-7, cd, want_unchanged=(method == "tncg" and j == segs - 1), seg=j)
    return s.get_factors()[0], n


def same_rows(A, ref, what):
    bad = np.flatnonzero((A != ref).any(axis=1))
    assert np.array_equal(A, ref), f"{what}: {len(bad)} of {len(ref)} rows differ in bits, first rows {bad[:8].tolist()}"


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def base(request):
    """the case's problem and its baseline: one session, one segment, one call"""
    case = request.param
    method, prec, k, maxupd, want = CASES[case]
    csr, csc, A0, B0 = problem(case)
    s = api.Session(csr, csc, A0.shape[0], DIMB, k, prec)
    A, n = a_half(s, case, A0, B0)
    plan = [name for name, _ in s.plan(1)]
    yield dict(case=case, csr=csr, csc=csc, A0=A0, B0=B0, A=A, n=n, s=s, plan=plan)
    s.close()


def test_the_plan_names_the_engines_of_the_case(base):
    for frag in CASES[base["case"]][4] if not KNOBS_SET else []:
        assert any(frag in name for name in base["plan"]), (frag, base["plan"])
    assert np.isfinite(base["A"]).all() and not base["A"][-1].any()        # (the empty last row)


@pytest.mark.parametrize("nseg", [2, 8])
def test_a_segments_one_by_one(base, nseg):
    s = base["s"]
    assert s.set_segments(1, nseg) == nseg
    try:
        A, n = a_half(s, base["case"], base["A0"], base["B0"], segs=nseg)
    finally:
        s.set_segments(1, 1)
    same_rows(A, base["A"], f"{nseg} segments one by one")
    assert n == base["n"]


def test_b_segments_in_one_call(base):
    s = base["s"]
    for nseg in (8, 5) if base["case"] == "tncg-f64-k100" else (8,):   # (k = 100 TNCG: eight team launches per segment -- five segments are 40)
        assert s.set_segments(1, nseg) == nseg
        try:
            A, n = a_half(s, base["case"], base["A0"], base["B0"])
            plan = [name for name, _ in s.plan(1)]
        finally:
            s.set_segments(1, 1)
        same_rows(A, base["A"], f"{nseg} segments in one call")
        assert n == base["n"]
        # (register instances may differ where a bin rides with another: compared without S)
        strip = lambda names: {re.sub(r"S=\d+", "S=*", x) for x in names}
        assert strip(plan) == strip(base["plan"]), sorted(strip(plan) ^ strip(base["plan"]))


def test_c_three_sharded_sessions(base):
    case = base["case"]
    method, prec, k, maxupd, _ = CASES[case]
    dimA = base["A0"].shape[0]
    cuts = [0, dimA // 7, dimA // 7 + dimA // 2 + 3, dimA]
    A, n = base["A0"].copy(), 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s = api.Session(base["csr"], base["csc"], dimA, DIMB, k, prec, shardA=(lo, hi))
        Ai, ni = a_half(s, case, base["A0"], base["B0"])
        s.close()
        A[lo:hi] = Ai[lo:hi]
        n += ni
    same_rows(A, base["A"], "three sharded sessions")
    assert n == base["n"]


def test_d_rows_in_reverse_order(base):
    import scipy.sparse as sp
    case = base["case"]
    method, prec, k, maxupd, _ = CASES[case]
    csr, dimA = base["csr"], base["A0"].shape[0]
    X = sp.csr_matrix((csr[0], csr[1].astype(np.int64), csr[2].astype(np.int64)), shape=(dimA, DIMB))
    csr2, csc2 = harness.process_data(X[::-1].tocoo(), prec)
    s = api.Session(csr2, csc2, dimA, DIMB, k, prec)
    A, n = a_half(s, case, np.ascontiguousarray(base["A0"][::-1]), base["B0"])
    s.close()
    same_rows(A[::-1], base["A"], "rows in reverse order")
    assert n == base["n"]


def test_e_filler_rows_in_two_register_classes(base):
    """5000 more rows of 20 nonzeros and 2500 of 300: those bins are then worth register launches of their own (plan_half: 4096 / 2048 rows) and the
    bins below ride with THEM -- another instance (S) for the same rows wherever `ride` holds, and it must not show in their bits"""
    import scipy.sparse as sp
    case = base["case"]
    method, prec, k, maxupd, _ = CASES[case]
    csr, dimA = base["csr"], base["A0"].shape[0]
    rng = np.random.default_rng(7)
    X = sp.csr_matrix((csr[0], csr[1].astype(np.int64), csr[2].astype(np.int64)), shape=(dimA, DIMB))
    fill_len = np.array([20] * 5000 + [300] * 2500)
    cols = np.concatenate([rng.choice(DIMB, size=n, replace=False) for n in fill_len])
    F = sp.csr_matrix((1.0 + np.floor(rng.gamma(1.0, 1.0, len(cols))), cols, np.concatenate([[0], np.cumsum(fill_len)])), shape=(len(fill_len), DIMB))
    csr2, csc2 = harness.process_data(sp.vstack([X, F]).tocoo(), prec)
    A0 = np.concatenate([base["A0"], harness.initialize_matrices(len(fill_len), DIMB, k, prec, 77)[0]])
    s = api.Session(csr2, csc2, A0.shape[0], DIMB, k, prec)
    A, _ = a_half(s, case, A0, base["B0"])
    plan = [name for name, _ in s.plan(1)]
    s.close()
    same_rows(A[:dimA], base["A"], "with 7500 filler rows")
    print(f"{case}: register instances with filler {sorted(p for p in set(plan) if 'reg' in p)}, without {sorted(p for p in set(base['plan']) if 'reg' in p)}")


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from tests.test_gpu_invariance import problem, CASES
from tests.test_gpu_parity import gpu_run
method, prec, k, maxupd, _ = CASES[{case!r}]
csr, csc, A0, B0 = problem({case!r})
A, B, _ = gpu_run(csr, csc, A0, B0, method, 1, k, maxupd=maxupd)
np.save({out!r}, np.concatenate([A.ravel().astype(np.float64), B.ravel().astype(np.float64)]))
"""


@pytest.mark.parametrize("case", ["tncg-f64-k100", "cg-f64-k50"])
def test_f_device_list_equals_one_device(tmp_path, case):
    res = {}
    for tag, env in (("one", {}), ("many", {"POISMF_HIP_DEVICES": "0,0,0", "POISMF_SHARD_COLSUM_MIN_ROWS": "1"})):
        out = str(tmp_path / f"{tag}.npy")
        e = dict(os.environ); e.pop("POISMF_HIP_DEVICES", None); e.update(env)
        subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, out=out, case=case)], check=True, env=e, cwd=ROOT, timeout=600)
        res[tag] = np.load(out)
    assert np.isfinite(res["one"]).all()
    bad = np.flatnonzero(res["one"] != res["many"])
    assert not len(bad), f"{len(bad)} entries differ between one device and the list 0,0,0"


def checker_a_half(case, csr, A0, B0, use_float=None):
    """the checker's A half from (A0, B0) with the baseline's parameters (tests/test_gpu_fullsize.py mirrors a session's half-sweep the same way);
    use_float: the checker's precision if not the case's (inputs converted)"""
    method, prec, k, maxupd, _ = CASES[case]
    uf = prec if use_float is None else use_float
    dt = H.dtype_of(uf)
    orc = H.checker(uf, method)
    l2, _, _ = harness.auto_defaults(method, k)
    A, F, data = A0.astype(dt), B0.astype(dt), csr[0].astype(dt)
    bs = orc.sum_by_cols(F)
    if method == "pg":
        real = (lambda v: float(np.float32(v))) if uf else float
        step = real(1e-7)
        cnst_div = real(1. / (1. + 2. * real(l2) * step))                   # ref: src/poismf.c:511, as api.Session.cnst_div
        cs = bs * np.asarray(-step, dt) * np.asarray(-step, dt)             # the A half scales the sums twice (quirk Q1, ref: src/poismf.c:573-577)
        with np.errstate(all="ignore"):
            orc.pg_iteration(A, F, data, csr[2], csr[1], cnst_div, cs, None, step, 1.0, maxupd)
    elif method == "cg":
        orc.cg_iteration(A, F, data, csr[2], csr[1], True, bs, l2, 1.0, maxupd)
    else:
        orc.tncg_iteration(A, F, False, data, csr[2], csr[1], bs, l2, 1.0, maxupd, True)
    return A, bs, l2


def test_the_baseline_against_the_checker(base):
    """Equal bits between wrong answers prove nothing: the baseline itself -- the A half from (A0, B0) -- against the checker's A half, by the
    suite's per-solver rules (tests/test_gpu_parity.py compare(), tests/test_gpu_regtile.py, tests/test_gpu_regpair.py), objectives being the
    half's own (tests/helpers.py, half_objective).  TNCG on doubles as tests/test_gpu_giant.py judges it: a converged run_poismf on one device
    -- the baseline's launches for the same rows -- against tncg_yardstick / tncg_bound.

    (Measured on an MI355X: after TWO whole iterations the fp32 checker's own left-to-right sums over a row of 20 000 nonzeros have moved it
    1.8e-4 (k = 50) / 3.3e-4 (k = 7) from the fp64 oracle, where the kernels are 5.5e-7 / 4.3e-7 from it: a two-iteration run_poismf does not
    meet the 1e-4 of tests/test_gpu_regtile.py against that checker on these rows.  What is judged here is the baseline the bit comparisons use.)"""
    from tests.test_gpu_parity import gpu_run
    case, csr, csc, A0, B0, A = (base[x] for x in ("case", "csr", "csc", "A0", "B0", "A"))
    method, prec, k, maxupd, _ = CASES[case]
    assert not A[-1].any()
    if method == "tncg" and not prec:
        Af, Bf, args = gpu_run(csr, csc, A0, B0, method, 2, k, maxupd=1500)
        assert np.isfinite(Af).all() and Af.min() >= 0 and not Af[-1].any()
        Ar, Br, orf, self_var = H.tncg_yardstick(prec, csr, csc, A0, B0, args)
        og = harness.poisson_objective(Af, Bf, csr, args["l2_reg"], args["l1_reg"], args["w_mult"])
        print(f"{case}: objective gpu {og:.10g} checker {orf:.10g} rel {abs(og - orf) / abs(orf):.3g} (reference flavours among themselves {self_var:.3g})")
        assert abs(og - orf) <= H.tncg_bound(self_var) * abs(orf), (abs(og - orf) / abs(orf), self_var)
        return
    Ar, bs, l2 = checker_a_half(case, csr, A0, B0)
    fo, fr = (H.half_objective(M, B0, csr[0], csr[1], csr[2], bs, l2) for M in (A, Ar))
    obj = abs(fo - fr) / abs(fr)
    print(f"{case}: A gpu vs checker {H.scaled_err(A, Ar):.3g}, objective of the half gpu {fo:.10g} checker {fr:.10g} rel {obj:.3g}")
    if method == "pg":
        assert np.isfinite(Ar).all() and np.isfinite(A).all()
        if prec:
            A64, _, _ = checker_a_half(case, csr, A0, B0, use_float=False)     # what the fp32 checker's own sums are worth on these rows
            print(f"{case}: gpu vs fp64 oracle {H.scaled_err(A, A64):.3g}, fp32 checker vs fp64 oracle {H.scaled_err(Ar, A64):.3g}")
            assert H.scaled_err(A, Ar) <= 1e-4                                 # long rows in fp32 (tests/test_gpu_regtile.py)
        else:
            assert H.scaled_err(A, Ar) <= 1e-12
    elif method == "cg":
        if prec:
            assert obj <= 5e-3                                                 # (compare(), fp32 mid-path)
        else:
            assert H.scaled_err(A, Ar) <= 5e-3 and obj <= 1e-8                 # (compare(), fp64 mid-path)
    else:
        # fp32 TNCG is chaotic in the reference itself: one-sided, as in tests/test_gpu_regtile.py and test_gpu_regpair.py
        assert np.isfinite(A).all() and A.min() >= 0
        assert fo <= fr + 1e-2 * abs(fr)
