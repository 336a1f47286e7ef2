"""The quad engine's tail (quad_eval.hpp): elements 48, 49 of a nonzero's factor row live once, in the lane that finishes the nonzero's
prediction -- one register pair per lane and batch of four steps --, not in a seventh register pair of every step.

The A half alone, PG on floats at k = 50, from (A0, B) through a session, with the hyper-parameters of tests/test_gpu_reg_diet.py (kw: the
gradient reaches the factors' bits):

  row length    0, 1, 15 | 16 | 17, 47 | 48 | 49, 63 | 64 | 65, 111 | 112 | 113, 128, 159 | 160: both sides of step and batch edges, and 81, 96,
                129, 144 so that Q = 6 and Q = 9 have rows too -- six rows of each behind two rows that keep every shard off row 0.  The whole
                session runs all of them on Q = 10; the rows of each instance also run on a shard of their own, whose plan names the
                instance (Q = 1 .. 10);
  item factors  (a) random positive; (b) nonzero only in dimensions 48 and 49 -- a lost or doubled tail is an error of order one (a lost one:
                a zero prediction and NaN), not of 1e-7; (c) zero in dimensions 48 and 49;
  maxupd        1 and 10.

Checked: against the oracle's A half (tests/test_gpu_invariance.py, checker_a_half, mirrors a session's half the same way) at the bound of
tests/test_gpu_reg_diet.py (1e-5, scaled), with the oracle's zeros; dimensions 48 and 49 of every row against the oracle's at that bound on
their own, scaled by these two columns alone; against the sixteen-lane engine (poismf_hip_debug_reg_quad_off) at the same bound; every instance
on a shard of its own gives the whole session's bits; three runs give the same bits.

Needs an MI355X."""
import functools

import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_reg_diet import kw, same_or_close
from tests.test_gpu_regtile import ragged_problem

pytestmark = pytest.mark.gpu

K = 50
DIMB = 300
LENGTHS = [0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 81, 96, 111, 112, 113, 128, 129, 144, 159, 160]
REPS = 6
LEAD = 2                                            # rows in front of every shard
ROWS = [160] * LEAD + [n for n in LENGTHS for _ in range(REPS)]
INSTANCES = tuple(range(1, 11))                     # every Q: each has a length of LENGTHS
FACTORS = ("positive", "tail_only", "no_tail")
CASES = [(f, maxupd) for f in FACTORS for maxupd in (1, 10)]
BOUND = 1e-5
L2, STEP = kw(K)["l2_reg"], kw(K)["step_size"]


def rows_of(Q):
    """[first, last + 1) of the rows whose length takes instance Q: 16 (Q - 1) < nnz <= 16 Q (and the empty ones with Q = 1)"""
    mine = [i for i, n in enumerate(LENGTHS) if 16 * (Q - 1) < n <= 16 * Q or (Q == 1 and n == 0)]
    assert mine and mine == list(range(mine[0], mine[-1] + 1)), Q
    return LEAD + mine[0] * REPS, LEAD + (mine[-1] + 1) * REPS


@functools.lru_cache(maxsize=None)
def problem(factors):
    csr, csc, A0, B0 = ragged_problem(ROWS, DIMB, K, True, seed=170)
    # (the reference's start is 0.3 + U[0, 0.01): entries that differ in the second digit, so that an element in another's place shows)
    rng = np.random.default_rng(171)
    A0 = rng.uniform(0.1, 0.5, A0.shape).astype(np.float32)
    B = rng.uniform(0.1, 0.5, B0.shape).astype(np.float32)
    if factors == "tail_only":
        B[:, :48] = 0
    elif factors == "no_tail":
        B[:, 48:] = 0
    return csr, csc, A0, B


def marked(maxupd):
    return [n for n, _ in api.debug_plan(np.array(ROWS + [0], dtype=np.uint32), K, DIMB, "pg", True, maxupd=maxupd, engines=True)]


def a_half(factors, maxupd, shardA=None):
    """the A half from (A0, B) on a session, of the shard's rows only: (A, launches of that half)"""
    csr, csc, A0, B = problem(factors)
    s = api.Session(csr, csc, A0.shape[0], DIMB, K, True, shardA=shardA)
    try:
        s.set_factors(A0, B)
        p = s.make_params("pg", L2, step_size=STEP, maxupd=maxupd)
        step = s.real(STEP)
        s.half_sweep(1, p, step, s.cnst_div(L2, step))
        A, B1 = s.get_factors()
        assert np.array_equal(B1.view(np.uint32), B.view(np.uint32))
        return A, [name for name, _ in s.plan(1)]
    finally:
        s.close()


def oracle_a_half(factors, maxupd):
    csr, csc, A0, B = problem(factors)
    orc = H.checker(True, "pg")
    A = A0.copy()
    step = float(np.float32(STEP))
    cnst_div = float(np.float32(1. / (1. + 2. * float(np.float32(L2)) * step)))            # as api.Session.cnst_div (ref: src/poismf.c:511)
    cs = orc.sum_by_cols(B) * np.float32(-step) * np.float32(-step)                          # the A half scales the sums twice (ref: src/poismf.c:573-577)
    with np.errstate(all="ignore"):
        orc.pg_iteration(A, B, csr[0], csr[2], csr[1], cnst_div, cs, None, step, 1.0, maxupd)
    return A


@functools.lru_cache(maxsize=None)
def runs(factors, maxupd):
    """the quad engine's result, the oracle's and the sixteen-lane engine's: computed once per case"""
    assert marked(maxupd) == ["half_sweep_reg_kernel<float,pg,S=40>[quad]"]
    A, plan = a_half(factors, maxupd)
    assert plan == ["half_sweep_reg_kernel<float,pg,S=40>"], plan
    assert api.reg_quad_off(True, True) is False
    try:
        assert marked(maxupd) == ["half_sweep_reg_kernel<float,pg,S=40>"]
        A16, _ = a_half(factors, maxupd)
    finally:
        api.reg_quad_off(True, False)
    return dict(quad=A, oracle=oracle_a_half(factors, maxupd), sixteen=A16)


@pytest.mark.parametrize("factors,maxupd", CASES)
def test_against_the_oracle(factors, maxupd):
    r = runs(factors, maxupd)
    A, Ar = r["quad"], r["oracle"]
    A0 = problem(factors)[2]
    lo = LEAD + REPS                                                                        # the first row with data behind the lead
    assert np.isfinite(Ar[:-1]).all() and (Ar[lo:-1] > 0).any(axis=1).all()                # the oracle itself: every row with data alive
    assert not A[-1].any() and not A[LEAD:lo].any()                                         # empty rows
    err = same_or_close(A, Ar, BOUND)
    err_tail = same_or_close(A[:, 48:], Ar[:, 48:], BOUND)                                  # scaled by the largest entry of these two columns
    moved = float(np.abs(Ar[lo:-1, 48:] - A0[lo:-1, 48:]).max() / np.abs(Ar[:, 48:]).max())
    print(f"quad tail, B {factors}, maxupd={maxupd}: scaled error A {err:.3g}, dimensions 48, 49 alone {err_tail:.3g} (the half moved them by up to {moved:.3g})")
    assert np.array_equal(A == 0, Ar == 0)                                                  # the clamp decides the same way
    if factors == "tail_only":
        assert moved > 1e-2                                                                 # the gradient is the tail's alone, and of order one


@pytest.mark.parametrize("factors,maxupd", CASES)
def test_against_the_sixteen_lane_engine(factors, maxupd):
    r = runs(factors, maxupd)
    err = same_or_close(r["quad"], r["sixteen"], BOUND)
    err_tail = same_or_close(r["quad"][:, 48:], r["sixteen"][:, 48:], BOUND)
    print(f"quad against sixteen lanes, B {factors}, maxupd={maxupd}: scaled difference A {err:.3g}, dimensions 48, 49 alone {err_tail:.3g}")


@pytest.mark.parametrize("factors,maxupd", CASES)
def test_every_instance_on_a_shard_of_its_own_gives_the_whole_runs_bits(factors, maxupd):
    A = runs(factors, maxupd)["quad"]
    for Q in INSTANCES:
        lo, hi = rows_of(Q)
        hi += Q == 10                                                                       # (the empty last row goes with the last shard)
        assert lo != 0
        Ai, plan = a_half(factors, maxupd, shardA=(lo, hi))
        assert plan == [f"half_sweep_reg_kernel<float,pg,S={4 * Q}>"], (Q, plan)
        assert np.array_equal(Ai[lo:hi].view(np.uint32), A[lo:hi].view(np.uint32)), Q


@pytest.mark.parametrize("factors", FACTORS)
def test_three_runs_give_the_same_bits(factors):
    A = runs(factors, 10)["quad"]
    for _ in range(2):
        A2, _ = a_half(factors, 10)
        assert np.array_equal(A.view(np.uint32), A2.view(np.uint32))
