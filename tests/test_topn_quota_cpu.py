"""CPU-side checks of the batched top-N with per-group quotas (include/poismf_hip.h section 1n): the header's define equals the api
constant, the three symbols are declared with the agreed parameter names and exported by every flavour; the C entry point answers 2 /
0 without a device on the malformed cases, and never 2 for a row the quotas leave short; the Python checks raise on the same cases
before any library call; the one scratch allocation stays inside the budget and never shrinks when an argument grows; and the
reference walk the GPU tests compare against gives hand-written answers."""
import os

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_gpu_topn_quota import quota_select, quota_walk, ranked
from tests.test_topn_batch_cpu import BAD as BAD_BATCH, NITEMS, NUSERS, K, _NoDeviceSession, _define, _fake_fitted, _params
from tests.test_topn_deep_cpu import SHORT

NAMES = ("poismf_hip_topn_quota", "poismf_hip_session_topn_quota", "poismf_hip_topn_quota_scratch_bytes")
GROUPS = [j % 7 for j in range(NITEMS)]

# section 1f's table; what is left after exclusion no longer matters
BAD = {c: v for c, v in BAD_BATCH.items() if c != "n-above-items-left"}
# (group_of, quota, n_groups or None for len(quota)): every one invalid for the C entry; "r" marks what only a signed index can say
BAD_GROUPS = {
    "group-of-null": (None, [1] * 7, None),
    "quota-null": (GROUPS, None, 7),
    "no-groups": (GROUPS, [1] * 7, 0),
    "group-id-at-n-groups": (GROUPS[:-1] + [7], [1] * 7, None),
    "group-id-above-n-groups": (GROUPS, [1] * 6, None),
    "r-negative-group-id": ([-1] + GROUPS[1:], [1] * 7, None),
    "r-negative-quota": (GROUPS, [1, 1, -1, 1, 1, 1, 1], None),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_header_declares_the_prototypes_and_the_constants_agree():
    assert _params("poismf_hip_session_topn_quota") == ("int", ["s", "users", "n_users", "n_top", "group_of", "n_groups", "quota", "exclude_seen",
                                                                "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_quota") == ("int", ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "group_of", "n_groups", "quota",
                                                        "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_quota_scratch_bytes") == ("size_t", ["n_users", "n_top", "dimB", "n_groups", "k"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_TOPN_QUOTA_MAX_ITEMS") == api.TOPN_QUOTA_MAX_ITEMS == 2 ** 24


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_quota(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def _c_call(flavour, users, n, excl, group_of=GROUPS, quota=(2,) * 7, n_groups=None, n_users=None, dimB=NITEMS):
    """poismf_hip_topn_quota itself through ctypes; index arrays in the flavour's sparse_ix"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    out = np.full((max(m, 1), max(n, 1)), 12345, it)
    sc = np.full((max(m, 1), max(n, 1)), -7.0, dt)
    p = api._ptr
    ip, ii = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    g = ix(group_of) if group_of is not None else None
    q = ix(quota) if quota is not None else None
    ng = n_groups if n_groups is not None else len(quota)
    rc = lib.poismf_hip_topn_quota(p(A), p(B), K, NUSERS, dimB, p(u), m, n, p(g) if g is not None else None, ng,
                                   p(q) if q is not None else None, p(ip) if ip is not None else None, p(ii) if ii is not None else None,
                                   p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))   # (a C caller has no row count to get wrong)
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, n, excl = BAD[case]
    rc, out, sc = _c_call(flavour, users, n, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour,case", [(f, c) for f in (False, True, "r") for c in sorted(BAD_GROUPS) if f == "r" or not c.startswith("r-")],
                         ids=lambda v: v if isinstance(v, str) else "df"[v])
def test_c_entry_returns_2_on_malformed_groups(flavour, case):
    group_of, quota, ng = BAD_GROUPS[case]
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, group_of=group_of, quota=quota, n_groups=ng)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_too_many_items(flavour):
    """dimB = 2^24 + 1 is refused before group_of is read (the arrays here are far shorter)"""
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, dimB=2 ** 24 + 1)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u = np.zeros(1, np.uint64)
    g = np.zeros(2, np.uint64)
    q = np.ones(1, np.uint64)
    out = np.zeros(1, np.uint64)
    p = api._ptr
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_quota(p(A), p(A), k, 2, 2, p(u), 1, 1, p(g), 1, p(q), None, None, p(out), None) == 2


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, _ = _c_call(flavour, [0], 5, None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_call(flavour, [0], 0, None, group_of=None, quota=None, n_groups=0, n_users=0)   # (nothing else matters then)
    assert rc == 0


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(SHORT) + ["every-quota-zero", "quotas-sum-below-n"])
def test_c_entry_short_rows_are_not_an_argument_error(flavour, case):
    """past the checks the call needs a device: 0 where there is one, 1 where there is none, never 2"""
    if case in SHORT:
        users, n, excl = SHORT[case]
        if n > api.TOPN_BATCH_MAX_N_TOP:
            n = api.TOPN_BATCH_MAX_N_TOP   # (n-above-items: 128 items are not there either once 200 are excluded)
            excl = ([0, 200, 400], list(range(200)) * 2)
        rc, _, _ = _c_call(flavour, users, n, excl)
    elif case == "every-quota-zero":
        rc, _, _ = _c_call(flavour, [0, 1], 5, None, quota=[0] * 7)
    else:
        rc, _, _ = _c_call(flavour, [0, 1], 10, None, quota=[1] * 7)
    assert rc in (0, 1)


# ---- Python ----
def test_topn_quota_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_quota([0, 1], group_of=GROUPS)


PY_BAD_GROUPS = {
    "group-of-missing": dict(group_of=None),
    "group-of-too-short": dict(group_of=GROUPS[:-1]),
    "group-of-too-long": dict(group_of=GROUPS + [0]),
    "negative-group-id": dict(group_of=[-1] + GROUPS[1:]),
    "fractional-group-id": dict(group_of=[0.5] * NITEMS),
    "quota-array-too-short": dict(group_of=GROUPS, quota=[1] * 6),
    "negative-quota": dict(group_of=GROUPS, quota=[1, 1, -1, 1, 1, 1, 1]),
    "negative-scalar-quota": dict(group_of=GROUPS, quota=-1),
    "quota-missing": dict(group_of=GROUPS, quota=None),
}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_quota(users, n, group_of=GROUPS, quota=2, exclude=excl)


@pytest.mark.parametrize("case", sorted(BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_quota(users, n, group_of=GROUPS, quota=2, exclude=excl)


@pytest.mark.parametrize("case", sorted(PY_BAD_GROUPS))
def test_malformed_groups_raise_before_the_device(case):
    kw = PY_BAD_GROUPS[case]
    with pytest.raises(ValueError):
        _fake_fitted(True).topN_quota([0, 1], 5, **kw)
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_quota([0, 1], 5, **kw)


def test_too_many_items_raise_before_the_device():
    s = _NoDeviceSession(True)
    s.dimB = api.TOPN_QUOTA_MAX_ITEMS + 1
    with pytest.raises(ValueError, match="limit of 16777216"):
        s.topn_quota([0, 1], 5, group_of=[0], quota=1)


def test_session_wrapper_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_quota([1, 5], 5, group_of=GROUPS, exclude_seen=True)


def test_python_checks_shape_the_arguments():
    """a scalar quota broadcasts over max(group_of) + 1 groups; an array's length is the number of groups; short rows are accepted"""
    u, g, q, indptr, indices = api._topn_quota_args([0, 1], 5, GROUPS, 3, None, NUSERS, NITEMS)
    assert u.dtype == g.dtype == q.dtype == np.uint64 and len(g) == NITEMS and q.tolist() == [3] * 7 and indptr is None and indices is None
    q = api._topn_quota_args([0, 1], 5, GROUPS, [0, 1, 2, 5, 2 ** 31, 1, 1, 9, 9], None, NUSERS, NITEMS)[2]
    assert q.tolist() == [0, 1, 2, 5, 2 ** 31, 1, 1, 9, 9]                 # (two groups without items)
    assert api._topn_quota_args([0, 1], 5, GROUPS, 2 ** 70, None, NUSERS, NITEMS)[2].tolist() == [2 ** 63] * 7
    for case in sorted(SHORT):
        users, n, excl = SHORT[case]
        got = api._topn_quota_args(users, min(n, 128), GROUPS, 1, excl, NUSERS, NITEMS)
        assert (got[3] is None) == (excl is None)
    assert api._topn_quota_args([], 5, GROUPS, 0, None, NUSERS, NITEMS)[2].tolist() == [0] * 7


# ---- scratch ----
@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_budget_and_never_shrinks(flavour):
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    assert budget == 256 << 20
    fn = api.load_library(flavour).poismf_hip_topn_quota_scratch_bytes
    tops, items, batch = (1, 128), (1, 10 ** 5, 2 ** 24), (1, 64, 4096, 10 ** 6, 10 ** 8)
    size = {}
    for n in tops:
        for dimB in items:
            for ng in (1, dimB):
                for m in batch:
                    b = size[n, dimB, ng, m] = int(fn(m, n, dimB, ng, 50))
                    assert 0 < b <= budget, (m, n, dimB, ng, b)
    for (n, dimB, ng, m), b in size.items():
        for bigger in ((tops[-1], dimB, ng, m), (n, items[-1], ng if ng == 1 else items[-1], m), (n, dimB, dimB, m), (n, dimB, ng, batch[-1])):
            assert size[bigger] >= b, ((n, dimB, ng, m), bigger)
        later = [size[n, dimB, ng, x] for x in batch]
        assert later == sorted(later)
        assert [size[n, x, 1, m] for x in items] == sorted(size[n, x, 1, m] for x in items)
    assert int(fn(64, 128, 1000, 1000, 50)) < (8 << 20)        # a small call does not pay for a large one
    assert max(size.values()) > (budget >> 1)                 # (the bound is not vacuous)
    assert int(fn(1, 1, 2 ** 24, 1, 50)) >= 2 * 4 * 2 ** 24    # the two maps, 32 bits per item each
    assert fn(10 ** 6, 10, 10 ** 5, 1000, 50) == fn(10 ** 6, 10, 10 ** 5, 1000, 512)


# ---- the reference walk of tests/test_gpu_topn_quota.py ----
def _answer(scores, excl, group_of, quota, n, select):
    items, s = ranked(np.asarray(scores, np.float32), excl)
    p = select(items, group_of, quota, n)
    return items[p].tolist(), s[p].tolist()


@pytest.mark.parametrize("select", [quota_walk, quota_select], ids=["counters", "in-group-ranks"])
def test_reference_walk_on_hand_written_cases(select):
    #          item   0    1    2    3    4    5    6    7
    scores = [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0]
    groups = [0, 0, 0, 1, 1, 2, 0, 2]
    # quota 1 everywhere: the best of each group, 0 (group 0), 3 (group 1), 5 (group 2); nothing is left for a fourth entry
    assert _answer(scores, [], groups, [1, 1, 1], 4, select) == ([0, 3, 5], [9.0, 6.0, 4.0])
    # quota 2, 1, 0: 0 and 1 of group 0, 3 of group 1, nothing of group 2; n = 2 stops the walk early
    assert _answer(scores, [], groups, [2, 1, 0], 8, select) == ([0, 1, 3], [9.0, 8.0, 6.0])
    assert _answer(scores, [], groups, [2, 1, 0], 2, select) == ([0, 1], [9.0, 8.0])
    # an excluded item frees its group's slot for the next item of the group: without item 0, item 1 is group 0's first
    assert _answer(scores, [0], groups, [1, 1, 1], 4, select) == ([1, 3, 5], [8.0, 6.0, 4.0])
    assert _answer(scores, [0, 1, 3], groups, [1, 1, 1], 4, select) == ([2, 4, 5], [7.0, 5.0, 4.0])
    # a tie at the quota boundary goes to the smaller item index: items 1 and 2 tie for group 0's second slot
    tied = [9.0, 7.0, 7.0, 6.0, 5.0, 4.0, 7.0, 2.0]
    assert _answer(tied, [], groups, [2, 1, 1], 8, select) == ([0, 1, 3, 5], [9.0, 7.0, 6.0, 4.0])
    assert _answer(tied, [1], groups, [2, 1, 1], 8, select) == ([0, 2, 3, 5], [9.0, 7.0, 6.0, 4.0])
    # a quota at or above n_top does not bind; one above every count (2^31) neither
    assert _answer(scores, [], groups, [8, 8, 8], 8, select)[0] == list(range(8))
    assert _answer(scores, [], groups, [2 ** 31, 2 ** 31, 0], 8, select)[0] == [0, 1, 2, 3, 4, 6]
    # everything excluded
    assert _answer(scores, list(range(8)), groups, [1, 1, 1], 3, select) == ([], [])


def test_the_two_references_agree_on_random_rows():
    rng = np.random.default_rng(0)
    for trial in range(50):
        dimB = int(rng.integers(1, 200))
        scores = rng.integers(0, 12, dimB).astype(np.float32)         # many ties
        n_groups = int(rng.integers(1, 12))
        groups = rng.integers(0, n_groups, dimB)
        quota = rng.integers(0, 4, n_groups)
        excl = np.flatnonzero(rng.random(dimB) < 0.2)
        n = int(rng.integers(1, 30))
        assert _answer(scores, excl, groups, quota, n, quota_walk) == _answer(scores, excl, groups, quota, n, quota_select)
