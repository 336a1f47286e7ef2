"""The used width of the float PG lane instances (lane_eval.hpp, KU_; plan.hpp, lane_used_width), without a device.

At k = 50 a factor row is 13 slots = 52 floats, two of them padding.  The lane instances of four register sets carry 50: which instance a
k selects is read from the plan (poismf_hip_debug_plan_widths marks a launch that is specialised on the used width "[KU=50]" behind its
name; the names themselves are unchanged), what the instances cost from the metadata of the built fp32 library.

CPU only: the library is cross-compiled, never run on a device here."""
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_gpu_regpair import READELF, _kernel_metadata

pytestmark = pytest.mark.skipif(not all(os.path.exists(build.lib_path(f)) for f in (False, True)), reason="the HIP libraries are not built")

DIMF = 100000
# row lengths of both halves of the headline (bench.py: item rows ~ Poisson(1000), user rows ~ 100) and every length class around them
LENGTHS = np.array(list(range(0, 2201)), dtype=np.uint32)
_LANE = re.compile(r"^half_sweep_lane_kernel<float,pg,KS=13,V=(\d+),A=0,L=0(?:\+(\d+))?,NW=(\d+),2/SIMD>(?:\[KU=(\d+)\])?$")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def lane_launches(k, widths=True):
    """[(V, LP, NW, KU)] of the fp32 PG lane launches the planner gives rows of 0 .. 2200 nonzeros at this k (PG with ten updates: the headline)"""
    out = []
    for name, _ in api.debug_plan(LENGTHS, k, DIMF, "pg", True, maxupd=10, widths=widths):
        if "lane_kernel" in name:
            m = _LANE.match(name)
            assert m, name
            out.append((int(m.group(1)), int(m.group(2) or 0), int(m.group(3)), int(m.group(4) or 0)))
    return out


def mangled(v, lp, nw, ku):
    """half_sweep_lane_kernel<float, K_PG = 3, KS = 13, LV, LA = 0, LL = 0, NW, SMALL = true, LP, TX = 0, KU>"""
    return f"_Z22half_sweep_lane_kernelIfLi3ELi13ELi{v}ELi0ELi0ELi{nw}ELb1ELi{lp}ELi0ELi{ku}EEv8HalfArgsIT_E"


def test_k50_selects_the_instances_of_the_used_width_and_no_other_k_does():
    got = lane_launches(50)
    assert sorted(got) == [(4, 0, 4, 50), (4, 16, 4, 50)], got          # rows of 513 .. 1024 and of 1025 .. 1088 nonzeros
    for k in (49, 51, 52):
        assert sorted(lane_launches(k)) == [(4, 0, 4, 0), (4, 16, 4, 0)], k
    assert lane_launches(64) == []                                          # 16 slots: no lane instance, as before
    for k in (49, 50, 51, 52, 64):
        # the mark is all that poismf_hip_debug_plan_widths adds: same launches, same rows, same names
        plain = api.debug_plan(LENGTHS, k, DIMF, "pg", True, maxupd=10)
        marked = api.debug_plan(LENGTHS, k, DIMF, "pg", True, maxupd=10, widths=True)
        assert [(re.sub(r"\[KU=\d+\]$", "", n), r) for n, r in marked] == plain, k
    # the other solvers and the double library have no such instance
    for method in ("cg", "tncg"):
        assert not any("[KU=" in n for n, _ in api.debug_plan(LENGTHS, 50, DIMF, method, True, maxupd=10, widths=True))
    assert not any("[KU=" in n for n, _ in api.debug_plan(LENGTHS, 50, DIMF, "cg", False, maxupd=10, widths=True))


def test_the_full_width_switch_selects_the_instances_that_carry_every_element():
    was = api.lane_full_width(True, True)
    try:
        assert was is False
        assert sorted(lane_launches(50)) == [(4, 0, 4, 0), (4, 16, 4, 0)]
    finally:
        api.lane_full_width(True, False)
    assert sorted(lane_launches(50)) == [(4, 0, 4, 50), (4, 16, 4, 50)]


def test_the_headlines_lane_instances_run_without_scratch_and_the_used_width_frees_eight_registers():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf here")
    meta = _kernel_metadata(build.lib_path(True))
    used = lane_launches(50)
    assert used
    for inst in used:
        vgpr, agpr, scratch = meta[mangled(*inst)]
        print(f"half_sweep_lane_kernel<float, pg, V={inst[0]}, LP={inst[1]}, NW={inst[2]}, KU={inst[3]}>: {vgpr} VGPRs, {agpr} AGPRs, {scratch} bytes of scratch")
        assert scratch == 0, (inst, scratch)
        assert vgpr + agpr <= 256, (inst, vgpr, agpr)                     # two waves per SIMD
    # the main instance (rows of 513 .. 1024 nonzeros): two registers per set and wave less than its sibling of all 52 elements
    narrow, full = meta[mangled(4, 0, 4, 50)], meta[mangled(4, 0, 4, 0)]
    assert full[0] - narrow[0] >= 8, (full, narrow)
