"""What every batched top-N and rank wrapper hands to the library, against the prototypes of include/poismf_hip.h: a recording
stand-in takes the library's place -- on a session as its `lib`, on host factors as what load_library returns -- and each call is
compared with the header's parameter list: the symbol, the number of arguments, the integers at the named positions, which optional
pointers are NULL, and what the users and exclusion pointers point at.  No device and no built library is needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

from poismf_amd import api
from tests.test_rank_include_cpu import _NoDeviceSession
from tests.test_topn_batch_cpu import K, NITEMS, NUSERS, _fake_fitted, _params


class _Recorder:
    """stands in for the loaded library: every attribute is a function that notes its name and arguments and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


USERS = [3, 0, 2]                                    # (inside rows 0..3, the stand-in session's shard of A)
EXCL = ([0, 1, 1, 3], [4, 0, 7])
INCL = ([0, 2, 4, 6], [1, 2, 3, 4, 5, 6])
TABLE, OF = ([0, 2, 5], [4, 9, 1, 2, 3]), [1, 0, 1]
TEST = ([0, 1, 2, 3], [3, 4, 5])
ONES = np.ones(NITEMS)
GROUPS = np.arange(NITEMS) % 7

# variant: (symbol stem, PoisMF method, Session method, n, keyword arguments, {header parameter: expected integer})
TOPN = {
    "batch": ("topn_batch", "topN_batch", "topn_batch", 5, {}, {}),
    "include": ("topn_include", "topN_batch", "topn_batch", 5, {"include": INCL}, {}),
    "shared": ("topn_shared", "topN_batch", "topn_batch", 5, {"include": TABLE, "include_of": OF}, {"n_lists": 2}),
    "deep": ("topn_deep", "topN_deep", "topn_deep", 200, {}, {}),
    "quota": ("topn_quota", "topN_quota", "topn_quota", 5, {"group_of": GROUPS, "quota": 2}, {"n_groups": 7}),
    "weighted": ("topn_weighted", "topN_weighted", "topn_weighted", 5, {"item_weight": ONES}, {}),
    "adjusted": ("topn_adjusted", "topN_adjusted", "topn_adjusted", 5, {"adjust": None}, {}),
    "diverse": ("topn_diverse", "topN_diverse", "topn_diverse", 5, {"pool": 20, "lam": 0.5, "item_norm": ONES}, {"pool": 20}),
}
# variant: (symbol stem, keyword arguments, {header parameter: expected integer})
RANK = {
    "batch": ("rank_batch", {}, {}),
    "include": ("rank_include", {"include": INCL}, {}),
    "shared": ("rank_shared", {"include": TABLE, "include_of": OF}, {"n_lists": 2, "unite_test": 0}),
    "shared-united": ("rank_shared", {"include": TABLE, "include_of": OF, "unite_test": True}, {"n_lists": 2, "unite_test": 1}),
}


def _read(pointer, n):
    """n uint64 entries through a pointer a wrapper passed (it keeps its array alive)"""
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint64)), (n,)).tolist()


def _the_call(rec, symbol, users, exclude, ints):
    """the one call the stand-in saw, as {header parameter: argument}, after the checks every wrapper shares"""
    assert [name for name, _ in rec.calls] == [symbol]
    args = rec.calls[0][1]
    names = _params(symbol)[1]
    assert len(args) == len(names), (symbol, len(args), names)
    got = dict(zip(names, args))
    for key, value in dict(ints, n_users=len(users)).items():
        assert isinstance(got[key], int) and got[key] == value, (symbol, key, got[key], value)
    assert _read(got["users"], len(users)) == users
    assert (got["excl_indptr"] is None) == (exclude is None) and (got["excl_indices"] is None) == (exclude is None)
    if exclude is not None:
        assert _read(got["excl_indptr"], len(users) + 1) == exclude[0]
        assert _read(got["excl_indices"], len(exclude[1])) == exclude[1]
    return got


def _on_host(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(api, "load_library", lambda use_float: rec)
    return rec, {"k": K, "dimA": NUSERS, "dimB": NITEMS}


def _outputs(variant):
    """every combination of the outputs a top-N variant can be asked for, as keyword arguments"""
    keys = ("output_score", "output_value") if variant == "diverse" else ("output_score",)
    return [dict(zip(keys, flags)) for flags in itertools.product((False, True), repeat=len(keys))]


def _check_outputs(got, result, out):
    assert (got["out_score"] is None) == (not out["output_score"])
    assert got["out_ix"] is not None and len(result) == (3 if "output_value" in out else 2)
    if "output_value" in out:
        assert (got["out_value"] is None) == (not out["output_value"])


@pytest.mark.parametrize("variant", sorted(TOPN))
def test_topn_on_host_factors(monkeypatch, variant):
    stem, method, _, n, kw, ints = TOPN[variant]
    for exclude, out in itertools.product((None, EXCL), _outputs(variant)):
        rec, lead = _on_host(monkeypatch)
        result = getattr(_fake_fitted(True), method)(USERS, n, exclude=exclude, **kw, **out)
        got = _the_call(rec, "poismf_hip_" + stem, USERS, exclude, dict(ints, n_top=n, **lead))
        assert "exclude_seen" not in got and "query_B" not in got
        _check_outputs(got, result, out)
        assert result[0].shape == (len(USERS), n)
        if variant == "diverse":
            assert got["lambda"] == 0.5


@pytest.mark.parametrize("variant", sorted(TOPN))
def test_topn_on_a_session(variant):
    stem, _, method, n, kw, ints = TOPN[variant]
    for exclude, seen, out in itertools.product((None, EXCL), (False, True), _outputs(variant)):
        rec = _Recorder()
        result = getattr(_NoDeviceSession(True, rec), method)(USERS, n, exclude_seen=seen, exclude=exclude, **kw, **out)
        extra = {"query_B": 0} if variant == "weighted" else {}
        got = _the_call(rec, "poismf_hip_session_" + stem, USERS, exclude, dict(ints, n_top=n, exclude_seen=int(seen), **extra))
        assert "dimA" not in got
        _check_outputs(got, result, out)
        if variant == "diverse":
            assert got["lambda"] == 0.5


def test_weighted_on_a_session_with_item_queries():
    """query_items: the queries are rows of B, so they may lie beyond the users; the flag stands in front of exclude_seen"""
    rec = _Recorder()
    queries = [NUSERS + 1, NITEMS - 1]
    _NoDeviceSession(True, rec).topn_weighted(queries, 5, item_weight=ONES, query_items=True)
    got = _the_call(rec, "poismf_hip_session_topn_weighted", queries, None, {"n_top": 5, "query_B": 1, "exclude_seen": 0})
    names = _params("poismf_hip_session_topn_weighted")[1]
    assert names.index("query_B") + 1 == names.index("exclude_seen") and got["out_score"] is None


@pytest.mark.parametrize("variant", sorted(RANK))
def test_ranks_on_host_factors(monkeypatch, variant):
    stem, kw, ints = RANK[variant]
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    for exclude in (None, EXCL):
        rec, lead = _on_host(monkeypatch)
        ranks, n_adm = api.rank_batch(A, B, USERS, TEST, exclude=exclude, **kw)
        got = _the_call(rec, "poismf_hip_" + stem, USERS, exclude, dict(ints, **lead))
        assert "exclude_seen" not in got and got["out_rank"] is not None and got["out_n_adm"] is not None
        assert _read(got["test_indptr"], len(USERS) + 1) == TEST[0] and _read(got["test_indices"], len(TEST[1])) == TEST[1]
        assert len(ranks) == len(TEST[1]) and len(n_adm) == len(USERS)


@pytest.mark.parametrize("variant", sorted(RANK))
def test_ranks_on_a_session(variant):
    stem, kw, ints = RANK[variant]
    for exclude, seen in itertools.product((None, EXCL), (False, True)):
        rec = _Recorder()
        _NoDeviceSession(True, rec).rank_batch(USERS, TEST, exclude_seen=seen, exclude=exclude, **kw)
        got = _the_call(rec, "poismf_hip_session_" + stem, USERS, exclude, dict(ints, exclude_seen=int(seen)))
        assert "dimA" not in got and got["out_rank"] is not None and got["out_n_adm"] is not None
        assert _read(got["test_indptr"], len(USERS) + 1) == TEST[0] and _read(got["test_indices"], len(TEST[1])) == TEST[1]


def test_no_users_reach_no_library(monkeypatch):
    """the early return stands before the library on both targets: nothing is called, the shapes are those of an answer"""
    rec, _ = _on_host(monkeypatch)
    sess = _NoDeviceSession(True, rec)
    nothing = ([0], [])
    for variant in sorted(TOPN):
        _, host, resident, n, kw, _ = TOPN[variant]
        kw = {"include": {"include": nothing}, "shared": {"include": TABLE, "include_of": []}}.get(variant, kw)   # (lists for no users)
        for result in (getattr(_fake_fitted(True), host)([], n, output_score=True, **kw),
                       getattr(sess, resident)([], n, output_score=True, exclude_seen=True, **kw)):
            assert result[0].shape == (0, n) and result[1].shape == (0, n)
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    for kw in ({},{"include": nothing}, {"include": TABLE, "include_of": []}, {"include": TABLE, "include_of": [], "unite_test": True}):
        for ranks, n_adm in (api.rank_batch(A, B, [], nothing, **kw), sess.rank_batch([], nothing, exclude_seen=True, **kw)):
            assert len(ranks) == 0 and len(n_adm) == 0
    assert rec.calls == []
