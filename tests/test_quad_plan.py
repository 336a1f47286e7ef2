"""Which plans take the quad engine (quad_eval.hpp; plan.hpp, reg_quad), without a device.

PG on floats at k = 50 holds a nonzero of a one-wave register row in four lanes instead of sixteen.  The plan keeps the names it had
(half_sweep_reg_kernel<float,pg,S=..>: existing tests compare them literally); poismf_hip_debug_plan_engines marks such a launch "[quad]" behind
its name.  Every other k, solver and precision, a session without the line-padded factor copy (POISMF_HIP_NO_PAD) and a process that has set
poismf_hip_debug_reg_quad_off keep the sixteen-lane engine.

CPU only: the library is cross-compiled, never run on a device here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from poismf_amd import api, build

pytestmark = pytest.mark.skipif(not all(os.path.exists(build.lib_path(f)) for f in (False, True)), reason="the HIP libraries are not built")

DIMF = 100000
# every length up to the multi-wave rows, and enough rows at the upper edge of each one-wave instance (16 Q nonzeros) that it gets a launch of its own
# (a bin of fewer than 4096 rows rides with the next longer instance)
LENGTHS = np.concatenate([np.arange(0, 400)] + [np.full(4200, n) for n in range(16, 161, 16)]).astype(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def reg_launches(k, method="pg", use_float=True, maxupd=10, **kw):
    """[(name, rows)] of the one-wave register launches of the plan, marks included"""
    return [(n, r) for n, r in api.debug_plan(LENGTHS, k, DIMF, method, use_float, maxupd=maxupd, engines=True, **kw) if "half_sweep_reg_kernel" in n]


def test_k50_fp32_pg_is_marked_and_keeps_its_names():
    for maxupd in (1, 10):
        marked = reg_launches(50, maxupd=maxupd)
        assert marked and all(n.endswith(">[quad]") for n, _ in marked), marked
        assert sorted({int(n.split("S=")[1].split(">")[0]) for n, _ in marked}) == list(range(4, 41, 4)), marked   # S = 4 Q, Q = 1 .. 10
        plain = api.debug_plan(LENGTHS, 50, DIMF, "pg", True, maxupd=maxupd)
        every = api.debug_plan(LENGTHS, 50, DIMF, "pg", True, maxupd=maxupd, engines=True)
        # the marks are all this listing adds: same launches, same rows, same names
        assert [(n[:-len("[quad]")] if n.endswith("[quad]") else n.split("[KU=")[0], r) for n, r in every] == plain
        assert not any("[quad]" in n for n, _ in plain)
    assert all(n.endswith("[quad]") for n, _ in reg_launches(50, w_mult=3.0))


def test_other_k_solvers_and_doubles_are_not_marked():
    for k in (49, 51, 52, 64):
        got = reg_launches(k)
        assert got and not any("[quad]" in n for n, _ in got), (k, got)
    for method in ("cg", "tncg"):
        assert not any("[quad]" in n for n, _ in api.debug_plan(LENGTHS, 50, DIMF, method, True, maxupd=10, engines=True)), method
    for method in ("pg", "cg", "tncg"):
        assert not any("[quad]" in n for n, _ in api.debug_plan(LENGTHS, 50, DIMF, method, False, maxupd=10, engines=True)), method


def test_the_debug_switch_removes_the_mark():
    was = api.reg_quad_off(True, True)
    try:
        assert was is False
        got = reg_launches(50)
        assert got and not any("[quad]" in n for n, _ in got), got
        names_off = [(n, r) for n, r in got]
    finally:
        assert api.reg_quad_off(True, False) is True
    on = reg_launches(50)
    assert [(n[:-len("[quad]")], r) for n, r in on] == names_off          # the same launches over the same rows, engine aside


def test_without_the_padded_copy_the_plan_is_unmarked():
    # (the knob is read once per process: a child of its own)
    code = ("import numpy as np; from poismf_amd import api; "
            "p = api.debug_plan(np.arange(0, 200, dtype=np.uint32), 50, 100000, 'pg', True, maxupd=10, engines=True); "
            "assert any('half_sweep_reg_kernel' in n for n, _ in p), p; assert not any('[quad]' in n for n, _ in p), p")
    env = dict(os.environ, POISMF_HIP_NO_PAD="1")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
