"""CPU-side checks of the sampled top-N (include/poismf_hip.h section 1w): the symbols are declared, listed and exported and the unit is
built; the C entry point answers 2 / 0 without a device; the Python calls raise before any library call and come back with the shapes
of an answer when there are no users."""
import ctypes as C

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_topn_batch_cpu import NITEMS, NUSERS, K, _NoDeviceSession, _define, _fake_fitted, _params

NAMES = ("poismf_hip_topn_sampled", "poismf_hip_session_topn_sampled", "poismf_hip_topn_sampled_scratch_bytes")
BAD = {                                   # name -> keyword arguments that must be refused
    "temperature-negative": dict(temperature=-0.5), "temperature-above-3": dict(temperature=3.0001), "temperature-nan": dict(temperature=float("nan")),
    "temperature-text": dict(temperature="1"), "n-zero": dict(n=0), "n-above-128": dict(n=129), "seed-negative": dict(seed=-1),
    "seed-above-64-bits": dict(seed=2 ** 64), "user-out-of-range": dict(users=[0, NUSERS]),
    "exclude-not-ascending": dict(exclude=([0, 2, 2], [5, 3])),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_symbols_and_unit():
    assert build.UNITS["topn_sampled"] == ("topn_sampled.hip", [])
    assert _params("poismf_hip_topn_sampled") == ("int", ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "temperature", "seed",
                                                          "excl_indptr", "excl_indices", "out_ix", "out_score", "out_key"])
    assert _params("poismf_hip_session_topn_sampled")[1][:7] == ["s", "users", "n_users", "n_top", "temperature", "seed", "exclude_seen"]
    assert _define("POISMF_HIP_TOPN_SAMPLED_MAX_ITEMS") == api.TOPN_SAMPLED_MAX_ITEMS and api.TOPN_SAMPLED_MAX_T == 3.0
    for flavour in (False, True, "r"):
        assert all(n in api.EXPORTED_SYMBOLS and getattr(api.load_library(flavour), n) is not None for n in NAMES)


@pytest.mark.parametrize("case", sorted(BAD))
def test_python_refuses_before_the_library(case):
    kw = {"users": [0, 1], "n": 5, **BAD[case]}
    with pytest.raises(ValueError):
        _fake_fitted(True).topN_sampled(kw.pop("users"), **kw)
    kw = {"users": [0, 1], "n": 5, **BAD[case]}
    with pytest.raises(ValueError):
        _NoDeviceSession(False).topn_sampled(kw.pop("users"), kw.pop("n"), **kw)


@pytest.mark.parametrize("args", [(0, 1.0), (129, 1.0), (5, -1e-9), (5, 3.5), (5, float("nan"))], ids=str)
def test_c_entry_returns_2_and_writes_nothing(args):
    n_top, T = args
    A, B, u, out = np.ones((NUSERS, K)), np.ones((NITEMS, K)), np.zeros(2, np.uint64), np.full((2, 129), 12345, np.uint64)
    p = api._ptr
    fn = api.load_library(False).poismf_hip_topn_sampled
    assert fn(p(A), p(B), K, NUSERS, NITEMS, p(u), 2, n_top, T, 7, None, None, p(out), None, None) == 2 and np.all(out == 12345)
    assert fn(p(A), p(B), K, NUSERS, NITEMS, p(u), 0, n_top, T, 7, None, None, p(out), None, None) == 0   # (no users: nothing else matters)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
def test_no_users_come_back_with_the_shapes_of_an_answer(use_float):
    dt = np.float32 if use_float else np.float64
    for got in (_fake_fitted(use_float).topN_sampled([], 7, output_score=True), _NoDeviceSession(use_float).topn_sampled([], 7, output_key=True)):
        assert [g.shape for g in got][0] == (0, 7) and got[0].dtype == np.uint64 and got[1].dtype == dt and got[2].dtype == dt
    fn = api.load_library(use_float).poismf_hip_topn_sampled_scratch_bytes
    assert all(0 < fn(m, n, d, 50) <= 256 << 20 for m in (1, 10 ** 7) for n in (1, 128) for d in (1, 2 ** 24))
