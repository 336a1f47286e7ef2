"""CPU-side checks of the batched top-N over include lists (include/poismf_hip.h section 1h): the header's constants and symbols,
the two testing aids (scratch size and slice length, no HIP call), every "returns 2" case of the contract through the C entry point on a
machine without a device, the same cases through the Python wrappers before anything device-side is loaded, and include=None
behaving as before."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_topn_include", "poismf_hip_session_topn_include", "poismf_hip_topn_include_scratch_bytes",
         "poismf_hip_topn_include_slice")
MERGE_MAX = 2048      # entries the merge step ranks at once (the issue's bound on slices x n_top)


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1))


def test_header_constants_and_symbols():
    assert _define("POISMF_HIP_TOPN_INCLUDE_MAX_ROW") == api.TOPN_INCLUDE_MAX_ROW == 2 ** 24
    assert api.TOPN_INCLUDE_MAX_ROW * 4 == (_define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20) // 4
    assert re.search(r"^#define\s+POISMF_HIP_TOPN_NONE\s+\(~\(sparse_ix\)0\)", open(HEADER).read(), re.M)
    assert api.TOPN_NONE == 2 ** 64 - 1
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_the_symbols(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_budget(flavour):
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    fn = api.load_library(flavour).poismf_hip_topn_include_scratch_bytes
    for args in [(1, 0, 1, 1, 1), (10 ** 6, 10 ** 8, 128, 10 ** 5, 50), (10 ** 9, 10 ** 11, 10, 2 ** 31 - 1, 512)]:
        b = int(fn(*args))
        print(args, b)
        assert 0 < b <= budget == 256 << 20, (args, b)
    assert int(fn(64, 6400, 10, 1000, 50)) < (8 << 20)   # a small call does not pay for a large one


@pytest.mark.parametrize("n_top", [1, 10, 128])
def test_slice_aid(n_top):
    fn = api.load_library(True).poismf_hip_topn_include_slice
    smin = int(fn(0, n_top))
    assert smin >= 64 and smin == int(fn(1, n_top)) == int(fn(smin, n_top))
    lens = sorted(set(range(0, 3000, 7)) | {int(x) for x in np.logspace(0, np.log10(api.TOPN_INCLUDE_MAX_ROW), 4000)}
                  | {api.TOPN_INCLUDE_MAX_ROW - 1, api.TOPN_INCLUDE_MAX_ROW})
    prev = 0
    for ln in lens:
        s = int(fn(ln, n_top))
        assert s >= smin and s >= prev, (ln, s, prev)
        assert -(-ln // s) * n_top <= MERGE_MAX, (ln, s)
        prev = s
    assert int(fn(api.TOPN_INCLUDE_MAX_ROW, 128)) > smin   # (the bound bites: long lists do get longer slices)


NUSERS, NITEMS, K = 6, 300, 3
FULL = ([0, 3, 6], [1, 2, 3, 4, 5, 6])

# (users, n, include as (indptr, indices) or None, exclude as (indptr, indices) or None): every one invalid
BAD = {
    "user-out-of-range": ([0, NUSERS], 5, FULL, None),
    "negative-user": ([-1, 0], 5, FULL, None),
    "include-item-out-of-range": ([0, 1], 5, ([0, 1, 2], [3, NITEMS]), None),
    "include-negative-item": ([0, 1], 5, ([0, 1, 2], [-2, 4]), None),
    "include-descending-row": ([0, 1], 5, ([0, 2, 4], [1, 2, 9, 7]), None),
    "include-repeated-item": ([0, 1], 5, ([0, 2, 4], [1, 2, 7, 7]), None),
    "include-indptr-decreases": ([0, 1], 5, ([0, 3, 2], [1, 2, 7]), None),
    "exclude-item-out-of-range": ([0, 1], 5, FULL, ([0, 1, 2], [3, NITEMS])),
    "exclude-descending-row": ([0, 1], 5, FULL, ([0, 2, 4], [1, 2, 9, 7])),
    "exclude-repeated-item": ([0, 1], 5, FULL, ([0, 2, 4], [1, 2, 7, 7])),
    "exclude-indptr-decreases": ([0, 1], 5, FULL, ([0, 3, 2], [1, 2, 7])),
    "n-zero": ([0, 1], 0, FULL, None),
    "n-above-limit": ([0, 1], 129, FULL, None),
}


def _c_include(flavour, users, n, incl, excl, n_users=None, k=K, dimB=NITEMS):
    """poismf_hip_topn_include itself through ctypes; index arrays in the flavour's sparse_ix.  Outputs are pre-filled."""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    kk = max(k, 1)
    A, B = np.ones((NUSERS, kk), dt), np.ones((NITEMS, kk), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    out = np.full((max(m, 1), max(n, 1)), 12345, it)
    sc = np.full((max(m, 1), max(n, 1)), -7.0, dt)
    p = api._ptr
    ip, ii = (ix(incl[0]), ix(incl[1])) if incl is not None else (None, None)
    ep, ei = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    rc = lib.poismf_hip_topn_include(p(A), p(B), k, NUSERS, dimB, p(u), m, n, p(ip) if ip is not None else None,
                                     p(ii) if ii is not None else None, p(ep) if ep is not None else None,
                                     p(ei) if ei is not None else None, p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, n, incl, excl = BAD[case]
    rc, out, sc = _c_include(flavour, users, n, incl, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_null_include_and_k(flavour):
    rc, out, sc = _c_include(flavour, [0, 1], 5, None, None)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)
    for k in (0, -1, 513 if flavour is True else 257):
        rc, out, sc = _c_include(flavour, [0, 1], 5, FULL, None, k=k)
        assert rc == 2 and np.all(out == 12345), k


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_c_entry_overlong_rows(flavour):
    """a row's length is refused from the row pointers alone (the indices are never reached), so small arrays do"""
    long_incl = ([0, api.TOPN_INCLUDE_MAX_ROW + 1, api.TOPN_INCLUDE_MAX_ROW + 1], [1, 2])
    rc, out, sc = _c_include(flavour, [0, 1], 5, long_incl, None, dimB=2 ** 25)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)
    limit = (_define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20) // 8    # section 1f: BUDGET_MB / 8 Mi entries
    long_excl = ([0, limit + 1, limit + 1], [1, 2])
    rc, out, sc = _c_include(flavour, [0, 1], 5, FULL, long_excl, dimB=2 ** 26)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, sc = _c_include(flavour, [0], 5, ([0, 1], [3]), None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_include(flavour, [0], 0, None, None, n_users=0)   # (nothing else matters then)
    assert rc == 0


def _fake_fitted(use_float):
    """a model that looks fitted without any fit having run (no device is touched)"""
    m = api.PoisMF(k=K, use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    m.nusers, m.nitems = NUSERS, NITEMS
    m.is_fitted = True
    return m


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self, use_float):
        self.lib = None
        self.use_float = use_float
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, 4), (0, NITEMS)
        self.h = None


PY_BAD = dict(BAD)
PY_BAD["include-wrong-rows"] = ([0, 1], 5, ([0, 1, 2, 3], [1, 2, 3]), None)
PY_BAD["include-overlong-row"] = ([0, 1], 5, ([0, api.TOPN_INCLUDE_MAX_ROW + 1, api.TOPN_INCLUDE_MAX_ROW + 1], [1, 2]), None)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(PY_BAD))
def test_model_wrapper_raises_before_the_device(use_float, case):
    users, n, incl, excl = PY_BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_batch(users, n, exclude=excl, include=incl)


@pytest.mark.parametrize("case", sorted(PY_BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, incl, excl = PY_BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_batch(users, n, exclude=excl, include=incl)


def test_session_wrapper_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_batch([1, 5], 5, exclude_seen=True, include=FULL)


def test_include_is_checked_like_exclude():
    """the same messages as for `exclude`; a dense array is refused; a stored zero stays a candidate"""
    with pytest.raises(ValueError, match="include: the item indices of a row must be strictly ascending"):
        _fake_fitted(True).topN_batch([0, 1], 5, include=([0, 2, 4], [1, 2, 9, 7]))
    with pytest.raises(ValueError, match="an item index of include is out of range"):
        _fake_fitted(True).topN_batch([0, 1], 5, include=([0, 1, 2], [3, NITEMS]))
    with pytest.raises(ValueError, match="include must be a SciPy sparse matrix"):
        _fake_fitted(True).topN_batch([0, 1], 5, include=np.ones((2, NITEMS)))
    X = sp.csr_matrix((np.array([1.0, 1.0, 1.0, 0.0, 1.0]), np.array([7, 2, 2, 5, 9]), np.array([0, 4, 5])), shape=(2, NITEMS))
    _, ip, ii, ep, ei = api._topn_include_args([0, 1], 128, X, None, NUSERS, NITEMS)   # (n above the list's length is fine)
    assert ip.tolist() == [0, 3, 4] and ii.tolist() == [2, 5, 7, 9] and ep is None and ei is None
    with pytest.raises(ValueError, match="rows for"):
        api._topn_include_args([0, 1, 2], 5, X, None, NUSERS, NITEMS)


def test_without_include_nothing_changes():
    """include=None: n above what exclusion leaves still raises, in the model and in the session"""
    excl = ([0, 0, 201], list(range(201)))
    with pytest.raises(ValueError, match="left after exclusion"):
        _fake_fitted(True).topN_batch([0, 1], 100, exclude=excl)
    with pytest.raises(ValueError, match="left after exclusion"):
        _NoDeviceSession(True).topn_batch([0, 1], 100, exclude=excl, include=None)
    with pytest.raises(ValueError, match="larger than the number of items"):
        api._topn_batch_args([0, 1], 100, None, NUSERS, 50)
