"""explain (include/poismf_hip.h section 1v) without a device: the symbols, the unit, the limits, and the wrappers' argument checks,
which stand before the library on host factors and on a session alike."""
import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_rank_include_cpu import _NoDeviceSession
from tests.test_serving_calls_cpu import USERS, _on_host
from tests.test_topn_batch_cpu import K, NITEMS, NUSERS, _define, _fake_fitted, _params

SEEN = ([0, 2, 2, 3], [1, 5, 7], [1.0, 2.0, 3.0])
PAGE = np.array([[1, 2], [3, 4], [5, api.TOPN_NONE]], np.uint64)


def test_symbols_unit_and_limits():
    for name in ("poismf_hip_explain", "poismf_hip_session_explain", "poismf_hip_explain_scratch_bytes"):
        assert name in api.EXPORTED_SYMBOLS and _params(name)[0].split()[0] in ("int", "size_t")
    assert build.UNITS["explain"][0] == "explain.hip"
    assert (api.EXPLAIN_MAX_M, api.EXPLAIN_MAX_QUERIES, api.EXPLAIN_MAX_ROW) == tuple(
        _define("POISMF_HIP_EXPLAIN_MAX_" + n) for n in ("M", "QUERIES", "ROW"))


# every one invalid: keyword arguments over a valid call
BAD = {
    "m-0": {"m": 0},
    "m-65": {"m": 65},
    "129-queries": {"items": np.zeros((3, 129), np.uint64)},
    "negative-scale": {"comp_scale": [1.0, -1.0, 1.0]},
    "nan-scale": {"comp_scale": [1.0, np.nan, 1.0]},
    "items-rows": {"items": PAGE[:2]},
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_wrappers_raise_before_the_library(monkeypatch, case):
    rec, _ = _on_host(monkeypatch)
    kw = dict({"items": PAGE, "m": 5, "comp_scale": None}, **BAD[case])
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    for call in (lambda: api.explain(A, B, USERS, seen=SEEN, **kw), lambda: _fake_fitted(True).explain(USERS, seen=SEEN, **kw),
                 lambda: _NoDeviceSession(True, rec).explain(USERS, **kw)):
        with pytest.raises(ValueError):
            call()
    assert rec.calls == []


def test_what_reaches_the_library_and_no_users_reach_none(monkeypatch):
    rec, dims = _on_host(monkeypatch)
    ix, val = _fake_fitted(True).explain(USERS, PAGE, SEEN, m=4, comp_scale=np.ones(K))
    assert [name for name, _ in rec.calls] == ["poismf_hip_explain"] and len(rec.calls[0][1]) == len(_params("poismf_hip_explain")[1])
    got = dict(zip(_params("poismf_hip_explain")[1], rec.calls[0][1]))
    assert dict(dims, n_users=3, n_q=2, m=4).items() <= got.items() and got["comp_scale"] is not None
    assert ix.shape == (3, 2, 4) and val.shape == (3, 2, 4) and val.dtype == np.float32
    del rec.calls[:]
    sess, none = _NoDeviceSession(True, rec), np.empty((0, 7), np.uint64)
    for ix, val in (api.explain(np.ones((NUSERS, K)), np.ones((NITEMS, K)), [], none, ([0], [], []), m=3), sess.explain([], none, m=3)):
        assert ix.shape == (0, 7, 3) and val.shape == (0, 7, 3)
    assert rec.calls == []
    sess.explain(USERS, PAGE)
    assert [name for name, _ in rec.calls] == ["poismf_hip_session_explain"] and len(rec.calls[0][1]) == len(_params("poismf_hip_session_explain")[1])
