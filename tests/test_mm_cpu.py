"""Method "mm" without a device: planned launch for launch as "pg" is (plan.hpp, plan_method), and the Python side knows its name.  CPU only."""
import os

import numpy as np
import pytest

from poismf_amd import api, build, harness

LENGTHS = np.concatenate([np.arange(0, 1400), [5000, 9000, 20000], np.full(4200, 100)]).astype(np.uint32)


@pytest.mark.skipif(not all(os.path.exists(build.lib_path(f)) for f in (False, True)), reason="the HIP libraries are not built")
@pytest.mark.parametrize("maxupd,w", [(1, 1.), (10, 1.), (10, 3.)])
@pytest.mark.parametrize("k", [3, 50, 100])
@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
def test_mm_is_planned_as_pg_is(use_float, k, maxupd, w):
    build.build()
    for kw in (dict(), dict(engines=True), dict(missing=True)):
        pg, mm = (api.debug_plan(LENGTHS, k, 100000, m, use_float, maxupd=maxupd, w_mult=w, **kw) for m in ("pg", "mm"))
        assert [(n.replace(",mm,", ",pg,"), r) for n, r in mm] == pg, kw
        assert kw.get("missing") or (mm and all(",mm," in n for n, _ in mm))


def test_the_name_is_known_and_an_unknown_one_refused():
    model = api.PoisMF(method="mm")
    assert api._METHOD["mm"] == 4 and (model.l2_reg_, model.niter_, model.maxupd_) == harness.auto_defaults("cg", 50)[:1] + (30, 10)
    with pytest.raises(ValueError):
        api.PoisMF(method="nope")
