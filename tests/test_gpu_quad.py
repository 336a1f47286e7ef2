"""The quad engine (quad_eval.hpp): PG on floats at k = 50 holds each nonzero of a one-wave register row in four lanes, sixteen nonzeros to a
step, ten instances Q = 1 .. 10 (rows of up to 16 Q nonzeros).

Small problems through the session, hyper-parameters under which the gradient reaches the factors' bits (kw of tests/test_gpu_reg_diet.py):

  row length  both sides of every step edge of the layout -- 0, 1, 15 | 16 | 17, 31 | 32 | 33, 47 | 48 | 49, 63 | 64 | 65, 79 | 80 | 81, 95 | 96 | 97,
              111 | 112 | 113, 127 | 128 | 129, 143 | 144 | 145, 159 | 160 -- six rows of each, behind two rows that keep every shard off row 0;
  maxupd      1 and 10; w_mult 1 and 3;
  start       exact zeros scattered over both factors and one all-zero row of A whose user has a single nonzero (a zero prediction, an infinite
              coefficient, NaN against the tile's zeros).

Checked: against the oracle at the bound tests/test_gpu_reg_diet.py holds PG on floats to (1e-5, scaled), with the oracle's zeros; against the
sixteen-lane engine in the same process (poismf_hip_debug_reg_quad_off) at the same bound -- the order of the sums differs, so not bit for bit;
every instance on a shard of its own (row_offset != 0) gives the whole session's bits; three runs give the same bits; without the line-padded
factor copy (POISMF_HIP_NO_PAD=1, a fresh process) the plan is unmarked and the result within the bound.

Needs an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from poismf_amd import api
from tests.test_gpu_parity import oracle_run, run_args
from tests.test_gpu_reg_diet import kw, same_or_close, session_run
from tests.test_gpu_regtile import ragged_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 50
DIMB = 300
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128, 129, 143, 144, 145, 159, 160]
REPS = 6
LEAD = 2                                            # rows in front of every shard
ROWS = [160] * LEAD + [n for n in LENGTHS for _ in range(REPS)]
CASES = [(1, 1.0), (10, 1.0), (1, 3.0), (10, 3.0)]
BOUND = 1e-5


def rows_of(Q):
    """[first, last + 1) of the rows whose length takes instance Q: 16 (Q - 1) < nnz <= 16 Q (and the empty ones with Q = 1)"""
    mine = [i for i, n in enumerate(LENGTHS) if 16 * (Q - 1) < n <= 16 * Q or (Q == 1 and n == 0)]
    assert mine == list(range(mine[0], mine[-1] + 1))
    return LEAD + mine[0] * REPS, LEAD + (mine[-1] + 1) * REPS


@functools.lru_cache(maxsize=None)
def problem():
    csr, csc, A0, B0 = ragged_problem(ROWS, DIMB, K, True, seed=150)
    for M, mul in ((A0, 7), (B0, 5)):               # exact zeros: three elements of every second row of either factor
        r = np.arange(0, len(M), 2)
        for off in (0, 3, 11):
            M[r, (mul * r + off) % K] = 0
    A0[LEAD + LENGTHS.index(1) * REPS] = 0           # a user with one nonzero
    return csr, csc, A0, B0


def args_of(maxupd, w):
    return run_args("pg", 1, K, maxupd=maxupd, w_mult=w, **kw(K))


def marked(maxupd, w):
    return [n for n, _ in api.debug_plan(np.array(ROWS + [0], dtype=np.uint32), K, DIMB, "pg", True, maxupd=maxupd, w_mult=w, engines=True)]


@functools.lru_cache(maxsize=None)
def runs(maxupd, w):
    """the quad engine's result, the oracle's and the sixteen-lane engine's: computed once per case"""
    csr, csc, A0, B0 = problem()
    args = args_of(maxupd, w)
    assert marked(maxupd, w) == ["half_sweep_reg_kernel<float,pg,S=40>[quad]"]
    A, B, plan = session_run(csr, csc, A0, B0, K, "pg", args)
    assert plan == ["half_sweep_reg_kernel<float,pg,S=40>"], plan
    Ar, Br = oracle_run(True, csr, csc, A0, B0, "pg", args)
    assert api.reg_quad_off(True, True) is False
    try:
        assert marked(maxupd, w) == ["half_sweep_reg_kernel<float,pg,S=40>"]
        A16, B16, _ = session_run(csr, csc, A0, B0, K, "pg", args)
    finally:
        api.reg_quad_off(True, False)
    return dict(quad=(A, B), oracle=(Ar, Br), sixteen=(A16, B16))


@pytest.mark.parametrize("maxupd,w", CASES)
def test_against_the_oracle(maxupd, w):
    r = runs(maxupd, w)
    (A, B), (Ar, Br) = r["quad"], r["oracle"]
    A0 = problem()[2]
    alive = np.isfinite(Ar).all(axis=1) & (Ar > 0).any(axis=1)
    # The item of the all-zero user gets a zero prediction in the B half, NaN in its whole row and, clamped, zeros; every user who has that item then
    # meets the same fate in the A half -- in the oracle too.  With 300 items that is a row of n nonzeros with probability n / 300, about 50 of the
    # 182 rows with data: at least half of them must be alive, and some of every instance.
    assert alive.sum() >= 0.5 * (len(ROWS) - REPS), alive.sum()
    for Q in range(1, 11):
        assert alive[slice(*rows_of(Q))].any(), Q
    assert not A[-1].any() and not A[LEAD:LEAD + REPS].any()                          # empty rows
    errA, errB = same_or_close(A, Ar, BOUND), same_or_close(B, Br, BOUND)
    zeros_kept = int(((Ar == 0) & (A0 == 0))[alive].sum())
    print(f"quad PG fp32 maxupd={maxupd} w={w}: scaled error A {errA:.3g} B {errB:.3g}; {alive.sum()} rows alive, {zeros_kept} planted zeros still zero")
    assert np.array_equal(A == 0, Ar == 0) and np.array_equal(B == 0, Br == 0)        # the clamp decides the same way


@pytest.mark.parametrize("maxupd,w", CASES)
def test_against_the_sixteen_lane_engine(maxupd, w):
    r = runs(maxupd, w)
    (A, B), (A16, B16) = r["quad"], r["sixteen"]
    errA, errB = same_or_close(A, A16, BOUND), same_or_close(B, B16, BOUND)
    print(f"quad against sixteen lanes, maxupd={maxupd} w={w}: scaled difference A {errA:.3g} B {errB:.3g}")


@pytest.mark.parametrize("maxupd,w", CASES)
def test_every_instance_on_a_shard_of_its_own_gives_the_whole_runs_bits(maxupd, w):
    csr, csc, A0, B0 = problem()
    A, B = runs(maxupd, w)["quad"]
    args = args_of(maxupd, w)
    for Q in range(1, 11):
        lo, hi = rows_of(Q)
        hi += Q == 10                                                                  # (the empty last row goes with the last shard)
        assert lo != 0
        Ai, Bi, plan = session_run(csr, csc, A0, B0, K, "pg", args, shardA=(lo, hi))
        assert plan == [f"half_sweep_reg_kernel<float,pg,S={4 * Q}>"], (Q, plan)
        assert np.array_equal(Ai[lo:hi].view(np.uint32), A[lo:hi].view(np.uint32)), Q
        assert np.array_equal(Bi.view(np.uint32), B.view(np.uint32)), Q


def test_three_runs_give_the_same_bits():
    csr, csc, A0, B0 = problem()
    A, B = runs(10, 1.0)["quad"]
    for _ in range(2):
        A2, B2, _ = session_run(csr, csc, A0, B0, K, "pg", args_of(10, 1.0))
        assert np.array_equal(A.view(np.uint32), A2.view(np.uint32)) and np.array_equal(B.view(np.uint32), B2.view(np.uint32))


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_quad as Q
names = Q.marked(10, 1.0)
assert names == ["half_sweep_reg_kernel<float,pg,S=40>"], names
csr, csc, A0, B0 = Q.problem()
A, B, plan = Q.session_run(csr, csc, A0, B0, Q.K, "pg", Q.args_of(10, 1.0))
assert plan == names, plan
np.savez({out!r}, A=A, B=B)
"""


def test_without_the_padded_copy_the_sixteen_lane_engine_runs(tmp_path):
    out = str(tmp_path / "nopad.npz")
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, out=out)], check=True, env=dict(os.environ, POISMF_HIP_NO_PAD="1"), cwd=ROOT, timeout=300)
    got = np.load(out)
    Ar, Br = runs(10, 1.0)["oracle"]
    same_or_close(got["A"], Ar, BOUND)
    same_or_close(got["B"], Br, BOUND)
    assert np.array_equal(got["A"] == 0, Ar == 0)
