"""The one-wave register kernels after their pass lost its no-op and loop-invariant instructions (reg_eval.hpp): PG on floats
takes the point unmasked and hands the gradient back instead of adding it to zeros; every fp32 instance exchanges the four groups' sums without
address arithmetic, folds a last batch of twelve steps with banked DPP adds, and sends the lanes without a slot to the zero row through the
gather's multiply-add.

Small PG fp32 problems through the session against the oracle, at the bound tests/helpers.py states for PG on floats (1e-5, scaled), with
hyper-parameters under which the gradient reaches the factors' bits (as in tests/test_gpu_lane_width.py; the benchmark's step of 1e-9 hides a
changed sum):

  k           50 (three idle lanes, a half-filled last slot), 49 and 52 (other fills of it), 64 (no idle lane: the gather's multiplier is never
              0), 4 (one slot, fifteen idle lanes);
  row length  0, 1, 4, 63 | 64 | 65, 80 | 81, 96 | 97, 111, 112 | 113, 128 | 129, 160: both sides of every batch of 64 nonzeros and of every
              instance, last batches of 4, 8, 12 and 16 steps; sixteen rows of each.  The planner lets a bin of fewer than 4096 rows ride with
              the next longer instance, so one session would run all of them on S = 40: the rows of each instance also run in a session of
              their own (a shard of A; its plan names the instance), and the shards together must give the whole session's bits;
  maxupd      1 and 10; w_mult = 3 once;
  start       exact zeros scattered over both factors (the gradient lifts them, or -- w_mult = 3 -- the clamp keeps some) and one all-zero row of
              A whose user has data: a zero prediction, an infinite coefficient, NaN against the tile's zeros -- entry for entry what the oracle makes of it.

One iteration, so that what the all-zero row does to its neighbours stays with its neighbours.  CG and TNCG on floats, rows of 97 .. 112
nonzeros (a last batch of twelve steps), against the oracle with the bounds of tests/test_gpu_parity.py: at k = 50, where these solvers take
the lane engine for such rows, and at k = 40, where they take the register instance S = 28 (the plan says so).  Three runs, the same bits.

Needs an MI355X."""
import functools

import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_parity import compare, oracle_run, run_args
from tests.test_gpu_regtile import ragged_problem

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 4, 63, 64, 65, 80, 81, 96, 97, 111, 112, 113, 128, 129, 160]
REPS = 16
DIMB = 1500
ROWS = [n for n in LENGTHS for _ in range(REPS)]   # row r has LENGTHS[r // REPS] nonzeros
INSTANCES = {4: (0, 3), 16: (3, 5), 20: (5, 7), 24: (7, 9), 28: (9, 12), 32: (12, 14), 36: (14, 15), 40: (15, 16)}   # S: the lengths [lo, hi) of LENGTHS it serves


def kw(k):
    """A step under which an update moves an entry by about a per cent of itself: the gradient of a 100-nonzero row is ~ sum_j x_j / pred_j F_j
    ~ 100 x 1.5 / (0.09 k) x 0.3 per entry, so the step goes with k (k = 50: 2e-4, step x gradient ~ 2e-3 against entries of 0.3).  A larger
    one overshoots (6e-6 k: k = 64 with ten updates ends in infinities, in the oracle too)."""
    return dict(l2_reg=1e2, step_size=4e-6 * k)


CASES = [(k, maxupd, 1.0) for k in (50, 49, 52, 64, 4) for maxupd in (1, 10)] + [(50, 10, 3.0)]


@functools.lru_cache(maxsize=None)
def problem(k):
    csr, csc, A0, B0 = ragged_problem(ROWS, DIMB, k, True, seed=100 + k)
    # exact zeros: one element of every second row of either factor, three where k allows (at k = 4 a row keeps three of its four entries, so
    # no prediction becomes zero by accident)
    for M, mul in ((A0, 7), (B0, 5)):
        r = np.arange(0, len(M), 2)
        for off in (0, 3, 11) if k > 16 else (0,):
            M[r, (mul * r + off) % k] = 0
    A0[LENGTHS.index(1) * REPS] = 0                 # a user with one nonzero
    return csr, csc, A0, B0


def session_run(csr, csc, A0, B0, k, method, args, shardA=None):
    """run_poismf's loop on a session (the B half, PG: half the step, the A half -- of the shard's rows only); (A, B, launches of the last A half)"""
    s = api.Session(csr, csc, A0.shape[0], B0.shape[0], k, True, shardA=shardA)
    try:
        s.set_factors(A0, B0)
        p = s.make_params(method, args["l2_reg"], args["l1_reg"], args["w_mult"], args["step_size"], args["limit_step"], args["maxupd"],
                          args["early_stop"], args["reuse_prev"])
        if shardA is None:
            assert s.run(p, args["niter"]) == 0
        else:
            step = args["step_size"]
            for _ in range(args["niter"]):
                step = s.sweep(p, step)
        A, B = s.get_factors()
        return A, B, [name for name, _ in s.plan(1)]
    finally:
        s.close()


def run_by_instance(csr, csc, A0, B0, k, args):
    """every instance on its own rows: (A put together from the shards, B -- the same from every shard)"""
    A, B = A0.copy(), None
    for S, (lo, hi) in INSTANCES.items():
        rows = (lo * REPS, hi * REPS + (S == 40))              # (the empty last row goes with the last shard)
        Ai, Bi, plan = session_run(csr, csc, A0, B0, k, "pg", args, shardA=rows)
        assert plan == [f"half_sweep_reg_kernel<float,pg,S={S}>"], (S, plan)
        A[rows[0]:rows[1]] = Ai[rows[0]:rows[1]]
        assert B is None or np.array_equal(B.view(np.uint32), Bi.view(np.uint32))
        B = Bi
    return A, B


def same_or_close(X, ref, bound):
    """non-finite entries in the same places with the same values; the others within `bound`, scaled by the largest finite entry"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(X), fin)
    assert np.array_equal(X[~fin], ref[~fin], equal_nan=True)
    err = H.scaled_err(np.where(fin, X, 0), np.where(fin, ref, 0))
    assert err <= bound, err
    return err


@pytest.mark.parametrize("k,maxupd,w", CASES)
def test_pg_fp32_against_the_oracle(k, maxupd, w):
    csr, csc, A0, B0 = problem(k)
    args = run_args("pg", 1, k, maxupd=maxupd, w_mult=w, **kw(k))
    Aw, Bw, plan = session_run(csr, csc, A0, B0, k, "pg", args)
    assert plan == ["half_sweep_reg_kernel<float,pg,S=40>"], plan
    A, B = run_by_instance(csr, csc, A0, B0, k, args)
    assert np.array_equal(A.view(np.uint32), Aw.view(np.uint32)) and np.array_equal(B.view(np.uint32), Bw.view(np.uint32))   # a row's bits do not depend on its instance
    Ar, Br = oracle_run(True, csr, csc, A0, B0, "pg", args)
    alive = np.isfinite(Ar).all(axis=1) & (Ar > 0).any(axis=1)
    assert alive.sum() >= 0.8 * (len(LENGTHS) - 1) * REPS, alive.sum()                                      # (rows of length 0 are zeroed)
    assert not A[-1].any() and not A[:REPS].any()                                                           # empty rows
    errA, errB = same_or_close(A, Ar, 1e-5), same_or_close(B, Br, 1e-5)
    zeros_kept = int(((Ar == 0) & (A0 == 0))[alive].sum())
    print(f"PG fp32 k={k} maxupd={maxupd} w={w}: scaled error A {errA:.3g} B {errB:.3g}; {alive.sum()} rows alive, {zeros_kept} planted zeros still zero")
    assert np.array_equal(A == 0, Ar == 0)          # the clamp decides the same way


def test_three_runs_give_the_same_bits():
    csr, csc, A0, B0 = problem(50)
    args = run_args("pg", 1, 50, maxupd=10, **kw(50))
    A, B, _ = session_run(csr, csc, A0, B0, 50, "pg", args)
    for _ in range(2):
        A2, B2, _ = session_run(csr, csc, A0, B0, 50, "pg", args)
        assert np.array_equal(A.view(np.uint32), A2.view(np.uint32)) and np.array_equal(B.view(np.uint32), B2.view(np.uint32))


@pytest.mark.parametrize("method,k", [("cg", 50), ("tncg", 50), ("cg", 40), ("tncg", 40)])
def test_cg_and_tncg_fp32_rows_with_a_last_batch_of_twelve_steps(method, k):
    csr, csc, A0, B0 = ragged_problem(list(range(97, 113)) * 8, DIMB, k, True, seed=61)
    args = run_args(method, 2, k, **(dict(maxupd=40) if method == "tncg" else {}))
    A, B, plan = session_run(csr, csc, A0, B0, k, method, args)
    if k == 40:
        assert f"half_sweep_reg_kernel<float,{method},S=28>" in plan, plan
    Ar, Br = oracle_run(True, csr, csc, A0, B0, method, args)
    assert not A[-1].any()
    compare(True, method, csr, args, A, B, Ar, Br, converged=False)
