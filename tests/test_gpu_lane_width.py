"""PG fp32 on the lane instances of four register sets (lane_eval.hpp), k = 49 .. 52: at k = 50 they are specialised on the used width -- 50 of
a factor row's 52 padded elements have a register (KU_) --, every other k runs the instances that carry all 52.  Ragged rows on either
side of the three hand-overs of these instances (512 | 513: from the register engine's eight waves; 1024 | 1025: to the partial LDS set;
1088 | 1089: back to the register engine), every share size class of the partial set among them:

  * against the oracle, with the bound tests/test_gpu_regtile.py holds long fp32 rows to (two summation orders over ~1000 nonzeros:
    ~sqrt(nnz) eps apart, 1e-4 scaled);
  * three runs, the same bits;
  * k = 50: the same bits from the instances that carry all 52 elements (poismf_hip_debug_lane_full_width) -- the terms the used width
    drops are exact zeros at the end of their chains.

Needs an MI355X."""
import functools

import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_parity import gpu_run, oracle_run
from tests.test_gpu_regtile import ragged_problem

pytestmark = pytest.mark.gpu

LENGTHS = [3, 100, 500, 511, 512, 513, 514, 600, 767, 900, 1000, 1023, 1024, 1025, 1026, 1027, 1028, 1029, 1040, 1041, 1055, 1056, 1072, 1087, 1088, 1089,
           1100, 1152]
DIMB = 6000
# Hyper-parameters under which the gradient REACHES the factors' bits: the Python defaults zero every entry within a sweep (zeros against
# zeros), and with the step of 1e-9 that other tests of these rows use an update moves an entry by a few ulp -- another order of the gradient's
# sums then changes nothing, the GPU agrees with the oracle to the last bit and a comparison of two instances could not fail.  With 3e-5 an
# update is ~1 % of an entry (step x gradient ~ 3e-5 x 100 against 0.3; the fixed point of a 1000-nonzero row is ~0.02, every entry stays positive).
KW = dict(l2_reg=1e3, step_size=3e-5, maxupd=10)


@functools.lru_cache(maxsize=None)
def _case(k):
    """the problem, one GPU run and the oracle's result: computed once per k"""
    csr, csc, A0, B0 = ragged_problem(LENGTHS, DIMB, k, True, seed=31 + k)
    A, B, args = gpu_run(csr, csc, A0, B0, "pg", 2, k, **KW)
    Ar, Br = oracle_run(True, csr, csc, A0, B0, "pg", args)
    return dict(k=k, problem=(csr, csc, A0, B0), gpu=(A, B), oracle=(Ar, Br))


@pytest.fixture(scope="module", params=[49, 50, 51, 52])
def case(request):
    return _case(request.param)


def test_the_plan_takes_these_rows_through_the_lane_instances(case):
    k = case["k"]
    names = [n for n, _ in api.debug_plan(LENGTHS + [0], k, DIMB, "pg", True, maxupd=10, widths=True)]
    mark = "[KU=50]" if k == 50 else ""
    for inst in ("L=0,NW=4,2/SIMD>", "L=0+16,NW=4,2/SIMD>"):
        assert f"half_sweep_lane_kernel<float,pg,KS=13,V=4,A=0,{inst}{mark}" in names, names


def test_against_the_oracle(case):
    (A, B), (Ar, Br) = case["gpu"], case["oracle"]
    assert np.isfinite(Ar).all() and Ar[:-1].min() > 0          # alive
    assert not A[-1].any()                                      # the empty row
    err = max(H.scaled_err(A, Ar), H.scaled_err(B, Br))
    print(f"PG fp32 k={case['k']}, rows of 3 .. 1152 nonzeros: scaled error against the oracle {err:.3g}")
    assert err <= 1e-4


def test_three_runs_give_the_same_bits(case):
    csr, csc, A0, B0 = case["problem"]
    A, B = case["gpu"]
    for _ in range(2):
        A2, B2, _ = gpu_run(csr, csc, A0, B0, "pg", 2, case["k"], **KW)
        assert np.array_equal(A, A2) and np.array_equal(B, B2)


def test_k50_gives_the_bits_of_the_instances_that_carry_all_52_elements():
    case = _case(50)
    csr, csc, A0, B0 = case["problem"]
    A, B = case["gpu"]
    assert api.lane_full_width(True, True) is False
    try:
        names = [n for n, _ in api.debug_plan(LENGTHS + [0], 50, DIMB, "pg", True, maxupd=10, widths=True)]
        assert any("lane_kernel" in n for n in names) and not any("[KU=" in n for n in names), names
        A2, B2, _ = gpu_run(csr, csc, A0, B0, "pg", 2, 50, **KW)
    finally:
        api.lane_full_width(True, False)
    assert np.array_equal(A.view(np.uint32), A2.view(np.uint32)) and np.array_equal(B.view(np.uint32), B2.view(np.uint32))
