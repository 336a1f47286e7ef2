"""What the quad engine's kernels (quad_eval.hpp, half_sweep_quad_kernel<Q>: PG on floats at k = 50, four lanes per nonzero) cost, read from
the metadata of the built fp32 library:

  * Q <= 7 (rows of up to 112 nonzeros): no scratch, at most 168 VGPRs -- three waves per SIMD;
  * Q = 8 (113 .. 128 nonzeros; 128 tile registers in the sixteen-lane engine, 112 here): no scratch; its VGPR count is printed -- 168 or
    fewer is a third wave per SIMD;
  * Q = 9, 10: no scratch and no more VGPRs than the sixteen-lane instances S = 36 / 40 they stand in for (216 / 226);
  * the sixteen-lane instances are all still there: every other k runs them (tests/test_reg_diet.py holds their budgets).

CPU only: the library is cross-compiled, never run on a device here."""
import os
import re

import pytest

from poismf_amd import build
from tests.test_gpu_regpair import READELF, _kernel_metadata

pytestmark = pytest.mark.skipif(not os.path.exists(build.lib_path(True)), reason="the fp32 HIP library is not built")

_QUAD = re.compile(r"^_Z22half_sweep_quad_kernelILi(\d+)EEv8HalfArgsIfE$")
_REG = re.compile(r"^_Z21half_sweep_reg_kernelIfLi3ELi(\d+)ELi16ELi1EEv8HalfArgsIT_E$")
SIXTEEN_LANE = {9: 216, 10: 226}      # VGPRs of half_sweep_reg_kernel<float, pg, S = 36 / 40> (profiles/r10/kernel_resource_usage.txt: 214, 226)


@pytest.fixture(scope="module")
def metadata():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf here")
    build.build()
    return _kernel_metadata(build.lib_path(True))


@pytest.fixture(scope="module")
def instances(metadata):
    out = {int(m.group(1)): v for m, v in ((_QUAD.match(name), v) for name, v in metadata.items()) if m}
    assert sorted(out) == list(range(1, 11)), sorted(out)
    for Q, (vgpr, agpr, scratch) in sorted(out.items()):
        print(f"half_sweep_quad_kernel<Q={Q}>: {vgpr} VGPRs, {agpr} AGPRs, {scratch} bytes of scratch")
    return out


@pytest.mark.parametrize("Q", range(1, 8))
def test_up_to_seven_steps_three_waves_and_no_scratch(instances, Q):
    vgpr, agpr, scratch = instances[Q]
    assert scratch == 0, f"Q = {Q}: {scratch} bytes of scratch per lane"
    assert agpr == 0 and vgpr <= 168, f"Q = {Q}: {vgpr} VGPRs + {agpr} AGPRs"


def test_eight_steps_no_scratch(instances):
    vgpr, agpr, scratch = instances[8]
    print(f"Q = 8: {vgpr} VGPRs ({'three' if vgpr + agpr <= 168 else 'two'} waves per SIMD)")
    assert scratch == 0 and agpr == 0, (vgpr, agpr, scratch)


@pytest.mark.parametrize("Q", sorted(SIXTEEN_LANE))
def test_nine_and_ten_steps_cost_no_more_than_the_sixteen_lane_instances(instances, Q):
    vgpr, agpr, scratch = instances[Q]
    assert scratch == 0, f"Q = {Q}: {scratch} bytes of scratch per lane"
    assert agpr == 0 and vgpr <= SIXTEEN_LANE[Q], f"Q = {Q}: {vgpr} VGPRs + {agpr} AGPRs, {SIXTEEN_LANE[Q]} in the sixteen-lane instance"


def test_the_sixteen_lane_instances_are_all_still_built(metadata):
    assert sorted(int(m.group(1)) for m in map(_REG.match, metadata) if m) == list(range(4, 41, 4))
