"""The quad engine's kernels (quad_eval.hpp, half_sweep_quad_kernel<Q>) with elements 48, 49 of a nonzero held once per batch of four steps --
a tile of 12 Q + 2 ceil(Q / 4) registers where it was 14 Q --, read from the metadata of the built fp32 library as tests/test_quad_resources.py
reads them:

  * no instance has more VGPRs than it had with the fourteen-register step (profiles/r10/kernel_resource_usage.txt: 118 / 132 / 146 / 160 /
    182 / 196 for Q = 5 .. 10; 55 / 69 / 83 / 97 for Q = 1 .. 4);
  * no instance uses scratch or AGPRs.

CPU only: the library is cross-compiled, never run on a device here."""
import os

import pytest

from poismf_amd import build
from tests.test_gpu_regpair import READELF, _kernel_metadata
from tests.test_quad_resources import _QUAD

pytestmark = pytest.mark.skipif(not os.path.exists(build.lib_path(True)), reason="the fp32 HIP library is not built")

FOURTEEN = {1: 55, 2: 69, 3: 83, 4: 97, 5: 118, 6: 132, 7: 146, 8: 160, 9: 182, 10: 196}   # VGPRs with seven register pairs per step


@pytest.fixture(scope="module")
def instances():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf here")
    build.build()
    out = {int(m.group(1)): v for m, v in ((_QUAD.match(name), v) for name, v in _kernel_metadata(build.lib_path(True)).items()) if m}
    assert sorted(out) == sorted(FOURTEEN), sorted(out)
    for Q, (vgpr, agpr, scratch) in sorted(out.items()):
        waves = min(8, 512 // ((vgpr + agpr + 7) // 8 * 8))
        print(f"half_sweep_quad_kernel<Q={Q}>: {vgpr} VGPRs ({FOURTEEN[Q]} before), {agpr} AGPRs, {scratch} bytes of scratch, {waves} waves per SIMD by registers")
    return out


@pytest.mark.parametrize("Q", sorted(FOURTEEN))
def test_no_more_registers_than_the_fourteen_register_step(instances, Q):
    vgpr, agpr, scratch = instances[Q]
    assert vgpr <= FOURTEEN[Q], f"Q = {Q}: {vgpr} VGPRs, {FOURTEEN[Q]} before"


@pytest.mark.parametrize("Q", sorted(FOURTEEN))
def test_no_scratch_and_no_agprs(instances, Q):
    vgpr, agpr, scratch = instances[Q]
    assert scratch == 0, f"Q = {Q}: {scratch} bytes of scratch per lane"
    assert agpr == 0, f"Q = {Q}: {agpr} AGPRs"
