"""CPU-side checks of the batched top-N over candidate lists shared between users (include/poismf_hip.h section 1i): the header's
constant and symbols, the scratch-size aid (no HIP call), every "returns 2" case of the contract through the C entry point on a machine
without a device, the same cases through the Python wrappers before anything device-side is loaded, the valid corner cases at the
argument check, and include_of=None behaving as before."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_topn_shared", "poismf_hip_session_topn_shared", "poismf_hip_topn_shared_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1))


def test_header_constant_and_symbols():
    assert _define("POISMF_HIP_TOPN_SHARED_MAX_CELLS") == api.TOPN_SHARED_MAX_CELLS == 2 ** 24
    assert api.TOPN_SHARED_MAX_CELLS * 4 == (_define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20) // 4
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
    fn = api.load_library(flavour).poismf_hip_topn_shared_scratch_bytes
    for args in [(1, 1, 0, 1, 1, 1), (10 ** 6, 8, 80000, 128, 10 ** 5, 50), (10 ** 9, 10 ** 6, 2 ** 24, 10, 2 ** 31 - 1, 512)]:
        b = int(fn(*args))
        print(args, b)
        assert 0 < b <= budget == 256 << 20, (args, b)
    assert int(fn(64, 1, 1000, 10, 1000, 50)) < (8 << 20)   # a small call does not pay for a large one


NUSERS, NITEMS, K = 6, 300, 3
TABLE = ([0, 3, 6], [1, 2, 3, 4, 5, 6])       # two lists of three items
OF = [0, 1]

# (users, n, table as (indptr, indices) or None, include_of or None, exclude as (indptr, indices) or None): every one invalid
BAD = {
    "user-out-of-range": ([0, NUSERS], 5, TABLE, OF, None),
    "negative-user": ([-1, 0], 5, TABLE, OF, None),
    "list-item-out-of-range": ([0, 1], 5, ([0, 1, 2], [3, NITEMS]), OF, None),
    "list-negative-item": ([0, 1], 5, ([0, 1, 2], [-2, 4]), OF, None),
    "list-descending-row": ([0, 1], 5, ([0, 2, 4], [1, 2, 9, 7]), OF, None),
    "list-repeated-item": ([0, 1], 5, ([0, 2, 4], [1, 2, 7, 7]), OF, None),
    "list-indptr-decreases": ([0, 1], 5, ([0, 3, 2], [1, 2, 7]), OF, None),
    "list-of-beyond-the-table": ([0, 1], 5, TABLE, [0, 2], None),
    "list-of-negative": ([0, 1], 5, TABLE, [-1, 0], None),
    "exclude-item-out-of-range": ([0, 1], 5, TABLE, OF, ([0, 1, 2], [3, NITEMS])),
    "exclude-descending-row": ([0, 1], 5, TABLE, OF, ([0, 2, 4], [1, 2, 9, 7])),
    "exclude-repeated-item": ([0, 1], 5, TABLE, OF, ([0, 2, 4], [1, 2, 7, 7])),
    "exclude-indptr-decreases": ([0, 1], 5, TABLE, OF, ([0, 3, 2], [1, 2, 7])),
    "n-zero": ([0, 1], 0, TABLE, OF, None),
    "n-above-limit": ([0, 1], 129, TABLE, OF, None),
}


def _c_shared(flavour, users, n, table, list_of, excl, n_users=None, k=K, dimB=NITEMS, n_lists=None):
    """poismf_hip_topn_shared itself through ctypes; index arrays in the flavour's sparse_ix.  Outputs are pre-filled."""
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
    lp, li = (ix(table[0]), ix(table[1])) if table is not None else (None, None)
    lof = ix(list_of) if list_of is not None else None
    ep, ei = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    G = n_lists if n_lists is not None else (len(lp) - 1 if lp is not None else 0)

    def opt(a):
        return p(a) if a is not None and len(a) else None

    rc = lib.poismf_hip_topn_shared(p(A), p(B), k, NUSERS, dimB, p(u), m, n, p(lp) if lp is not None else None, opt(li), G,
                                    p(lof) if lof is not None else None, p(ep) if ep is not None else None, opt(ei), p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, n, table, lof, excl = BAD[case]
    rc, out, sc = _c_shared(flavour, users, n, table, lof, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_null_arguments_no_lists_and_k(flavour):
    for table, lof, G in ((None, OF, 2), (TABLE, None, 2), (TABLE, OF, 0)):
        rc, out, sc = _c_shared(flavour, [0, 1], 5, table, lof, None, n_lists=G)
        assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0), (table, lof, G)
    for k in (0, -1, 513 if flavour is True else 257):
        rc, out, sc = _c_shared(flavour, [0, 1], 5, TABLE, OF, None, k=k)
        assert rc == 2 and np.all(out == 12345), k


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_c_entry_overlong_table_and_exclusion_row(flavour):
    """lengths are refused from the row pointers alone (the indices are never reached), so small arrays do: one row over the limit,
    two rows that are over it only together, and an exclusion row over section 1f's limit"""
    cells = api.TOPN_SHARED_MAX_CELLS
    rc, out, sc = _c_shared(flavour, [0, 1], 5, ([0, cells + 1, cells + 1], [1, 2]), OF, None, dimB=2 ** 25)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)
    half = cells // 2 + 1
    rc, out, sc = _c_shared(flavour, [0, 1], 5, ([0, half, 2 * half], [1, 2]), OF, None, dimB=2 ** 25)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)
    limit = (_define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20) // 8    # section 1f: BUDGET_MB / 8 Mi entries
    rc, out, sc = _c_shared(flavour, [0, 1], 5, TABLE, OF, ([0, limit + 1, limit + 1], [1, 2]), dimB=2 ** 26)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)


def test_python_refuses_a_table_over_the_limit(monkeypatch):
    """every row is admissible, the table as a whole is not (the limit lowered so that a small table shows it)"""
    api._topn_shared_args([0, 1], 5, TABLE, OF, None, NUSERS, NITEMS)
    monkeypatch.setattr(api, "TOPN_SHARED_MAX_CELLS", 5)
    with pytest.raises(ValueError, match="more than 5 indices"):
        api._topn_shared_args([0, 1], 5, TABLE, OF, None, NUSERS, NITEMS)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, sc = _c_shared(flavour, [0], 5, ([0, 1], [3]), [0], None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_shared(flavour, [0], 0, None, None, None, n_users=0)   # (nothing else matters then)
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
PY_BAD["list-of-wrong-length"] = ([0, 1], 5, TABLE, [0, 1, 0], None)
PY_BAD["list-of-not-integers"] = ([0, 1], 5, TABLE, [0.0, 1.0], None)
PY_BAD["list-of-int-beyond-the-table"] = ([0, 1], 5, TABLE, 2, None)
PY_BAD["list-of-negative-int"] = ([0, 1], 5, TABLE, -1, None)
PY_BAD["list-of-a-float"] = ([0, 1], 5, TABLE, 1.0, None)
PY_BAD["list-of-without-a-table"] = ([0, 1], 5, None, OF, None)
PY_BAD["table-without-rows"] = ([0, 1], 5, ([0], []), OF, None)
PY_BAD["table-dense"] = ([0, 1], 5, np.ones((2, NITEMS)), OF, None)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(PY_BAD))
def test_model_wrapper_raises_before_the_device(use_float, case):
    users, n, table, lof, excl = PY_BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_batch(users, n, exclude=excl, include=table, include_of=lof)


@pytest.mark.parametrize("case", sorted(PY_BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, table, lof, excl = PY_BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_batch(users, n, exclude=excl, include=table, include_of=lof)
    with pytest.raises(ValueError):
        api._topn_shared_args(users, n, table, lof, excl, NUSERS, NITEMS)


def test_session_wrapper_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_batch([1, 5], 5, exclude_seen=True, include=TABLE, include_of=OF)


def test_valid_corner_cases_pass_the_argument_check():
    """G = 1; an empty list; a list nobody refers to; n above every list; include_of as one int; a sparse table with a stored zero"""
    u, lp, li, lof, ep, ei = api._topn_shared_args([3, 0, 3], 128, ([0, 2], [4, 9]), 0, None, NUSERS, NITEMS)
    assert lp.tolist() == [0, 2] and li.tolist() == [4, 9] and lof.tolist() == [0, 0, 0] and lof.dtype == np.uint64 and ep is None and ei is None
    table = ([0, 0, 2, 5], [4, 9, 1, 2, 3])   # list 0 is empty, list 2 has no user
    u, lp, li, lof, ep, ei = api._topn_shared_args([0, 1, 2], 100, table, np.array([1, 0, 1], np.int32), ([0, 1, 1, 2], [4, 0]), NUSERS, NITEMS)
    assert lp.tolist() == [0, 0, 2, 5] and lof.tolist() == [1, 0, 1] and ep.tolist() == [0, 1, 1, 2] and ei.tolist() == [4, 0]
    X = sp.csr_matrix((np.array([1.0, 1.0, 1.0, 0.0, 1.0]), np.array([7, 2, 2, 5, 9]), np.array([0, 4, 5])), shape=(2, NITEMS))
    _, lp, li, lof, _, _ = api._topn_shared_args(np.arange(5), 10, X, [1, 1, 0, 0, 1], None, NUSERS, NITEMS)
    assert lp.tolist() == [0, 3, 4] and li.tolist() == [2, 5, 7, 9] and lof.tolist() == [1, 1, 0, 0, 1]
    _, lp, _, lof, _, _ = api._topn_shared_args([], 10, X, [], None, NUSERS, NITEMS)   # (no users)
    assert len(lof) == 0 and len(lp) == 3
    # ... and through the C check on a machine without a device these are not refused as arguments: rc 1 (no device) or 0, never 2
    for flavour in (False, True, "r"):
        rc, _, _ = _c_shared(flavour, [0, 1, 2], 100, table, [1, 0, 1], ([0, 1, 1, 2], [4, 0]))
        assert rc in (0, 1)


def test_without_include_of_nothing_changes():
    """include_of=None: `include` is a list per user, and a table with G != m rows still raises the existing error"""
    for call in (lambda **kw: _fake_fitted(True).topN_batch([0, 1, 2], 5, **kw), lambda **kw: _NoDeviceSession(True).topn_batch([0, 1, 2], 5, **kw)):
        with pytest.raises(ValueError, match="include has 2 rows for 3 users"):
            call(include=TABLE)
        with pytest.raises(ValueError, match="include has 2 rows for 3 users"):
            call(include=TABLE, include_of=None)
        with pytest.raises(ValueError, match="include has 2 rows for 3 users"):
            call(include=sp.csr_matrix((2, NITEMS)))
    excl = ([0, 0, 201], list(range(201)))
    with pytest.raises(ValueError, match="left after exclusion"):
        _fake_fitted(True).topN_batch([0, 1], 100, exclude=excl)
    with pytest.raises(ValueError, match="left after exclusion"):
        _NoDeviceSession(True).topn_batch([0, 1], 100, exclude=excl, include=None, include_of=None)
