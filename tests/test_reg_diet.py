"""What the one-wave PG fp32 register kernels (reg_eval.hpp, half_sweep_reg_kernel<float, pg, S, 16, 1>) cost, read from the metadata of the built
fp32 library: the pass over the tile lost its no-op and loop-invariant instructions, and no instance may have paid for that
with a wave per SIMD or with scratch.

  * S <= 28 (rows of up to 112 nonzeros, the bulk of a 100-nonzero-per-row matrix): no scratch, at most 168 VGPRs -- three waves per SIMD;
  * S = 32, 36, 40: no more VGPRs and no more scratch than before the change (profiles/r08/kernel_resource_usage.txt).

CPU only: the library is cross-compiled, never run on a device here."""
import os
import re

import pytest

from poismf_amd import build
from tests.test_gpu_regpair import READELF, _kernel_metadata

pytestmark = pytest.mark.skipif(not os.path.exists(build.lib_path(True)), reason="the fp32 HIP library is not built")

_REG = re.compile(r"^_Z21half_sweep_reg_kernelIfLi3ELi(\d+)ELi16ELi1EEv8HalfArgsIT_E$")
BEFORE = {32: 187, 36: 216, 40: 227}      # VGPRs, all without scratch


@pytest.fixture(scope="module")
def instances():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf here")
    build.build()
    out = {}
    for name, (vgpr, agpr, scratch) in _kernel_metadata(build.lib_path(True)).items():
        m = _REG.match(name)
        if m:
            out[int(m.group(1))] = (vgpr, agpr, scratch)
    assert sorted(out) == list(range(4, 41, 4)), sorted(out)
    for S, (vgpr, agpr, scratch) in sorted(out.items()):
        print(f"half_sweep_reg_kernel<float, pg, S={S}>: {vgpr} VGPRs, {agpr} AGPRs, {scratch} bytes of scratch")
    return out


@pytest.mark.parametrize("S", [4, 8, 12, 16, 20, 24, 28])
def test_instances_up_to_28_steps_keep_three_waves_and_no_scratch(instances, S):
    vgpr, agpr, scratch = instances[S]
    assert scratch == 0, f"S = {S}: {scratch} bytes of scratch per lane"
    assert agpr == 0 and vgpr <= 168, f"S = {S}: {vgpr} VGPRs + {agpr} AGPRs"


@pytest.mark.parametrize("S", sorted(BEFORE))
def test_longer_instances_cost_no_more_than_before(instances, S):
    vgpr, agpr, scratch = instances[S]
    assert scratch == 0, f"S = {S}: {scratch} bytes of scratch per lane"
    assert agpr == 0 and vgpr <= BEFORE[S], f"S = {S}: {vgpr} VGPRs + {agpr} AGPRs, {BEFORE[S]} before"
