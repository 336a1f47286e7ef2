"""The step-paired register tile of PG on floats (reg_eval.hpp, PAIR_): the tile held as register pairs of two consecutive steps,
dots of a step pair in one v_pk_mul + three v_pk_fma, the axpy accumulated as (even steps, odd steps).

GPU tests (marked gpu): rows on either side of every tile size (16 .. 160 nonzeros in steps of 16, i.e. S = 4 .. 40 steps of four
nonzeros), with odd and even step counts and one to three nonzeros, for PG, CG and TNCG on floats against the oracle with the
tolerances of tests/test_gpu_regtile.py; three runs of the same rows giving the same bits.

CPU test: the one-wave PG fp32 register instances up to S = 28 (rows of up to 112 nonzeros, the bulk of a 100-nonzero-per-row
matrix) keep zero scratch and at least three waves per SIMD, read from the code objects of the built library."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from poismf_amd import build as hip_build
from poismf_amd import harness
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

# 1 .. 13 nonzeros (one to four steps), then around every tile size E: E - 5, E - 4 (one step short, the other parity), E - 1, E,
# E + 1 (next tile), E + 4
PAIR_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13] + [n for e in range(16, 161, 16) for n in (e - 5, e - 4, e - 1, e, e + 1, e + 4)]


def _problem(k, seed=21):
    from tests.test_gpu_regtile import ragged_problem
    return ragged_problem(PAIR_LENGTHS, 3000, k, True, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("method,k", [("pg", 50), ("pg", 64), ("pg", 7), ("cg", 50), ("tncg", 50)])
def test_fp32_rows_at_every_tile_edge(method, k):
    from tests.test_gpu_parity import compare, gpu_run, oracle_run
    csr, csc, A0, B0 = _problem(k)
    kw = dict(maxupd=40) if method == "tncg" else {}
    A, B, args = gpu_run(csr, csc, A0, B0, method, 2, k, **kw)
    Ar, Br = oracle_run(True, csr, csc, A0, B0, method, args)
    assert not A[-1].any()   # the empty row
    if method == "pg" and np.isfinite(Ar).all():
        assert np.isfinite(A).all() and np.isfinite(B).all()
        assert H.scaled_err(A, Ar) <= 1e-4 and H.scaled_err(B, Br) <= 1e-4
    elif method == "tncg":
        # fp32 TNCG is chaotic in the reference itself: one-sided, as in test_gpu_regtile
        assert np.isfinite(A).all() and np.isfinite(B).all() and A.min() >= 0 and B.min() >= 0
        og = harness.poisson_objective(A, B, csr, args["l2_reg"], args["l1_reg"], args["w_mult"])
        orf = harness.poisson_objective(Ar, Br, csr, args["l2_reg"], args["l1_reg"], args["w_mult"])
        assert og <= orf + 1e-2 * abs(orf)
    else:
        compare(True, method, csr, args, A, B, Ar, Br, converged=False)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [50, 64])
def test_pg_fp32_paired_rows_repeat_bit_for_bit(k):
    from tests.test_gpu_parity import gpu_run
    csr, csc, A0, B0 = _problem(k, seed=23)
    runs = [gpu_run(csr, csc, A0, B0, "pg", 2, k)[:2] for _ in range(3)]
    A, B = runs[0]
    assert np.isfinite(A).all() and np.isfinite(B).all() and A.any()
    for A2, B2 in runs[1:]:
        assert np.array_equal(A, A2) and np.array_equal(B, B2)


def _kernel_metadata(lib):
    """{mangled kernel name: (vgpr_count, agpr_count, private_segment_fixed_size)} from the AMDGPU metadata notes of every gfx950
    code object in the library"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmf_isa_guard", os.path.join(ROOT, "scripts", "isa_guard.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    out = {}
    for image in g.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        # one YAML mapping per kernel; the fields come in alphabetical order, .agpr_count first
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
            pr = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if name and vg and pr:
                out[name.group(1)] = (int(vg.group(1)), int(block.split("\n", 1)[0].strip() or 0), int(pr.group(1)))
    return out


def test_pg_fp32_register_instances_up_to_28_steps_keep_three_waves_without_scratch():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf here")
    lib = hip_build.lib_path(True)
    if not os.path.exists(lib):
        pytest.skip("the fp32 library is not built")
    meta = _kernel_metadata(lib)
    # half_sweep_reg_kernel<float, K_PG = 3, S, 16, 1>
    pat = re.compile(r"^_Z21half_sweep_reg_kernelIfLi3ELi(\d+)ELi16ELi1EEv8HalfArgsIT_E$")
    seen = {}
    for name, (vgpr, agpr, scratch) in meta.items():
        m = pat.match(name)
        if m and int(m.group(1)) <= 28:
            seen[int(m.group(1))] = (vgpr, agpr, scratch)
    assert sorted(seen) == [4, 8, 12, 16, 20, 24, 28], sorted(seen)
    for S, (vgpr, agpr, scratch) in sorted(seen.items()):
        regs = (vgpr + 3) // 4 * 4 + agpr
        waves = 512 // ((regs + 7) // 8 * 8)
        assert scratch == 0, f"S = {S}: {scratch} bytes of scratch per lane"
        assert waves >= 3, f"S = {S}: {vgpr} VGPRs + {agpr} AGPRs, {waves} waves per SIMD"
