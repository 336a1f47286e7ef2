"""CPU-side checks of the batched ranks among per-user include lists (include/poismf_hip.h section 1j): the header declares the
three prototypes with the agreed parameter names, every library flavour exports them and the constants match poismf_amd.api; the
one scratch allocation of a call stays inside the budget the header states; every invalid input answers 2 from the C entry point
with nothing written, and raises from the Python wrappers, before anything reaches a device; the device-free union helper of
eval_ranking(include=) against np.union1d; and include=None still reaches the entry points of section 1g."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_rank_include", "poismf_hip_session_rank_include", "poismf_hip_rank_include_scratch_bytes")
NUSERS, NITEMS, K = 6, 300, 3


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _params(name):
    text = open(HEADER).read()
    m = re.search(r"^POISMF_HIP_API\s+([\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, f"{name} is not declared"
    return " ".join(m.group(1).split()), [re.match(r".*?(\w+)$", " ".join(p.split())).group(1) for p in m.group(2).split(",")]


def _define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(0x[0-9a-fA-F]+|\d+)", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1), 0)


# ---- 1. the boundary --------------------------------------------------------------------------------------------------------------

def test_header_declares_the_prototypes():
    ret, names = _params("poismf_hip_rank_include")
    assert ret == "int"
    assert names == ["A", "B", "k", "dimA", "dimB", "users", "n_users", "test_indptr", "test_indices", "incl_indptr", "incl_indices",
                     "excl_indptr", "excl_indices", "out_rank", "out_n_adm"]
    ret, names = _params("poismf_hip_session_rank_include")
    assert ret == "int"
    assert names == ["s", "users", "n_users", "test_indptr", "test_indices", "incl_indptr", "incl_indices", "exclude_seen", "excl_indptr",
                     "excl_indices", "out_rank", "out_n_adm"]
    ret, names = _params("poismf_hip_rank_include_scratch_bytes")
    assert ret == "size_t" and names == ["n_users", "n_test_cells", "n_incl_cells", "dimB", "k"]
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_RANK_INCLUDE_SLICE") == api.RANK_INCLUDE_SLICE and api.RANK_INCLUDE_SLICE % 64 == 0
    assert _define("POISMF_HIP_RANK_INCLUDE_GROUP") == api.RANK_INCLUDE_GROUP
    assert _define("POISMF_HIP_TOPN_INCLUDE_MAX_ROW") == api.TOPN_INCLUDE_MAX_ROW
    assert _define("POISMF_HIP_RANK_BATCH_MAX_ROW") == api.RANK_BATCH_MAX_ROW
    assert _define("POISMF_HIP_RANK_EXCLUDED") == api.RANK_EXCLUDED


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_rank_include(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


# ---- 2. the scratch ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_stated_budget(flavour):
    """the size both entry points allocate (one allocation per call), against the figure in the header's own text: up to 10^6 users,
    10^7 held-out cells and 10^9 candidates"""
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    assert budget == 256 << 20
    fn = api.load_library(flavour).poismf_hip_rank_include_scratch_bytes
    kmax = 512 if flavour else 256
    users = sorted({1, 2, 63, 64, 65, 1000, 4096, 10 ** 5, 262144, 262145, 10 ** 6} | {int(x) for x in np.logspace(0, 6, 19)})
    test_per_user = [0, 1, 10, 127, 128, 129, 1000]
    incl_per_user = [0, 1, 100, 1023, 1024, 1025, 10 ** 4]
    items = [1, 64, 3000, 10 ** 5, 2 ** 31 - 1]
    worst = 0
    for m in users:
        for c in test_per_user:
            for n in incl_per_user:
                for dimB in items:
                    for k in (1, 50, kmax):
                        b = int(fn(m, m * c, m * n, dimB, k))
                        assert 0 < b <= budget, (m, c, n, dimB, k, b)
                        worst = max(worst, b)
    for m, c, n in ((10 ** 6, 10 ** 7, 10 ** 9), (10 ** 6, 10 ** 7, 10 ** 8), (4096, 65536 * 4096, 2 ** 24 * 4096), (1, 65536, 2 ** 24)):
        for dimB in (10 ** 5, 2 ** 31 - 1):
            b = int(fn(m, c, n, dimB, 50))
            assert 0 < b <= budget, (m, c, n, dimB, b)
            worst = max(worst, b)
    # a small call does not pay for a large one
    assert int(fn(64, 640, 64 * 1000, 3000, 50)) < (8 << 20)
    assert worst > (budget >> 2)   # (the bound is not vacuous: large calls do use a good part of it)


# ---- 3. invalid input ------------------------------------------------------------------------------------------------------------------

# (users, test, include, exclude), lists as (indptr, indices): every one invalid
OK_T, OK_I = ([0, 1, 2], [3, 4]), ([0, 2, 4], [3, 9, 4, 7])
BAD = {
    "user-out-of-range": ([0, NUSERS], OK_T, OK_I, None),
    "negative-user": ([-1, 0], OK_T, OK_I, None),
    "test-item-out-of-range": ([0, 1], ([0, 1, 2], [3, NITEMS]), OK_I, None),
    "include-item-out-of-range": ([0, 1], OK_T, ([0, 2, 4], [3, 9, 4, NITEMS]), None),
    "include-negative-item": ([0, 1], OK_T, ([0, 2, 4], [-3, 9, 4, 7]), None),
    "exclude-item-out-of-range": ([0, 1], OK_T, OK_I, ([0, 1, 2], [3, NITEMS])),
    "include-unsorted-row": ([0, 1], OK_T, ([0, 2, 4], [9, 3, 4, 7]), None),
    "include-repeated-item": ([0, 1], OK_T, ([0, 2, 4], [3, 9, 7, 7]), None),
    "test-unsorted-row": ([0, 1], ([0, 2, 4], [1, 2, 9, 7]), OK_I, None),
    "exclude-unsorted-row": ([0, 1], OK_T, OK_I, ([0, 2, 4], [1, 2, 9, 7])),
    "include-decreasing-indptr": ([0, 1], OK_T, ([0, 2, 1], [3, 9]), None),
    "test-decreasing-indptr": ([0, 1], ([0, 2, 1], [1, 2]), OK_I, None),
    "include-wrong-rows": ([0, 1], OK_T, ([0, 1, 2, 3], [1, 2, 3]), None),
    "test-wrong-rows": ([0, 1], ([0, 1, 2, 3], [1, 2, 3]), OK_I, None),
}
NO_ROW_COUNT = {"include-wrong-rows", "test-wrong-rows"}   # (a C caller has no row count to get wrong)


def _c_call(flavour, users, test, incl, excl, n_users=None, k=K, null_incl=False):
    """poismf_hip_rank_include itself through ctypes; index arrays in the flavour's sparse_ix"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, max(k, 1)), dt), np.ones((NITEMS, max(k, 1)), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    tp, ti, ip, ii = ix(test[0]), ix(test[1]), ix(incl[0]), ix(incl[1])
    rank = np.full(max(len(ti), 1), 12345, np.uint32)
    n_adm = np.full(max(m, 1), 54321, np.uint32)
    p = api._ptr
    ep, ei = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    rc = lib.poismf_hip_rank_include(p(A), p(B), k, NUSERS, NITEMS, p(u), m, p(tp), p(ti), None if null_incl else p(ip), p(ii),
                                     p(ep) if ep is not None else None, p(ei) if ei is not None else None, p(rank), p(n_adm))
    return rc, rank, n_adm


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, test, incl, excl = BAD[case]
    rc, rank, n_adm = _c_call(flavour, users, test, incl, excl)
    assert rc == 2
    assert np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_null_include_indptr(flavour):
    rc, rank, n_adm = _c_call(flavour, [0, 1], OK_T, OK_I, None, null_incl=True)
    assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, rank, n_adm = _c_call(flavour, [0], ([0, 1], [3]), ([0, 1], [3]), None, n_users=0)
    assert rc == 0 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour,kmax", [(False, 256), (True, 512), ("r", 256)], ids=["d", "f", "r"])
def test_c_entry_k_out_of_range(flavour, kmax):
    for k in (0, -1, kmax + 1):
        rc, rank, n_adm = _c_call(flavour, [0, 1], OK_T, OK_I, None, k=k)
        assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


def _overlong():
    """one user whose include row is one entry over the limit (134 MB of indices: built once)"""
    n = api.TOPN_INCLUDE_MAX_ROW + 1
    return n, np.zeros(1, np.uint64), np.array([0, 1], np.uint64), np.zeros(1, np.uint64), np.array([0, n], np.uint64), np.arange(n, dtype=np.uint64)


def test_overlong_include_row():
    """through the C entry (flavours d and f share the index type; r's int indices are checked the same way by the same code) and
    through the Python wrapper"""
    n, u, tp, ti, ip, ii = _overlong()
    p = api._ptr
    for flavour, dt in ((True, np.float32), (False, np.float64)):
        A, B = np.ones((1, 1), dt), np.ones((n, 1), dt)
        rank, n_adm = np.full(1, 12345, np.uint32), np.full(1, 54321, np.uint32)
        lib = api.load_library(flavour)
        assert lib.poismf_hip_rank_include(p(A), p(B), 1, 1, n, p(u), 1, p(tp), p(ti), p(ip), p(ii), None, None, p(rank), p(n_adm)) == 2
        assert rank[0] == 12345 and n_adm[0] == 54321
    ip32, ii32 = ip.astype(np.int32), ii.astype(np.int32)
    A, B = np.ones((1, 1), np.float64), np.ones((n, 1), np.float64)
    rank, n_adm = np.full(1, 12345, np.uint32), np.full(1, 54321, np.uint32)
    u32, tp32, ti32 = u.astype(np.int32), tp.astype(np.int32), ti.astype(np.int32)
    assert api.load_library("r").poismf_hip_rank_include(p(A), p(B), 1, 1, n, p(u32), 1, p(tp32), p(ti32), p(ip32), p(ii32), None, None, p(rank),
                                                         p(n_adm)) == 2
    assert rank[0] == 12345 and n_adm[0] == 54321
    with pytest.raises(ValueError, match="longer"):
        api.rank_batch(np.ones((1, 1), np.float32), np.ones((n, 1), np.float32), [0], (tp, ti), include=(ip, ii))


def test_overlong_test_row():
    n = api.RANK_BATCH_MAX_ROW + 1
    row = np.arange(n)
    B = np.ones((n, 2), np.float32)
    with pytest.raises(ValueError, match="longer"):
        api.rank_batch(np.ones((2, 2), np.float32), B, [0], ([0, n], row), include=([0, n], row))


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self, use_float, lib=None):
        self.lib = lib
        self.use_float = use_float
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, 4), (0, NITEMS)
        self.h = None


@pytest.mark.parametrize("case", sorted(BAD))
def test_python_wrappers_raise_before_the_device(case):
    users, test, incl, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).rank_batch(users, test, exclude=excl, include=incl)
    for dt in (np.float32, np.float64):
        with pytest.raises(ValueError):
            api.rank_batch(np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt), users, test, exclude=excl, include=incl)


def _x(rows, cols, shape=(NUSERS, NITEMS)):
    return sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=shape)


def _fake_fitted(use_float):
    m = api.PoisMF(k=K, use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    m.nusers, m.nitems = NUSERS, NITEMS
    m.is_fitted = True
    return m


X_OK = _x([0, 1, 1], [5, 7, 9])
BAD_EVAL_INCLUDE = {
    "matrix-wrong-shape": (_x([0], [5], (NUSERS, NITEMS - 1)), None),
    "matrix-fewer-rows": (_x([0], [5], (NUSERS - 1, NITEMS)), None),
    "pair-wrong-rows": (([0, 1, 2, 3], [1, 2, 3]), [0, 1]),
    "pair-item-out-of-range": (([0, 1, 2], [3, NITEMS]), [0, 1]),
    "pair-unsorted-row": (([0, 2, 4], [1, 2, 9, 7]), [0, 1]),
    "pair-decreasing-indptr": (([0, 2, 1], [1, 2]), [0, 1]),
    "not-a-list": (np.ones((NUSERS, NITEMS)), None),
}


@pytest.mark.parametrize("case", sorted(BAD_EVAL_INCLUDE))
def test_eval_ranking_include_raises_before_the_device(case):
    incl, users = BAD_EVAL_INCLUDE[case]
    for use_float in (False, True):
        with pytest.raises(ValueError):
            _fake_fitted(use_float).eval_ranking(X_OK, include=incl, users=users)
    with pytest.raises(ValueError):
        _NoDeviceSession(True).eval_ranking(X_OK, include=incl, users=users, exclude_seen=False)


def test_session_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).rank_batch([1, 5], ([0, 1, 2], [3, 4]), exclude_seen=True, include=([0, 1, 2], [3, 4]))   # (user 5: rows 0..3)


# ---- 4. the union helper -----------------------------------------------------------------------------------------------------------

def _rows(rng, m, n_items, most):
    rows = [np.sort(rng.choice(n_items, int(rng.integers(0, most + 1)), replace=False)) for _ in range(m)]
    return rows, (np.concatenate(([0], np.cumsum([len(r) for r in rows]))), np.concatenate(rows) if m else np.empty(0, np.int64))


@pytest.mark.parametrize("m", [0, 1, 7, 200])
def test_union_helper_against_union1d(m):
    rng = np.random.default_rng(m)
    ra, a = _rows(rng, m, 60, 25)
    rb, b = _rows(rng, m, 60, 6)
    if m >= 7:
        ra[3] = rb[3].copy()                        # the same row twice, an empty row against a full one, both empty
        ra[4], rb[5] = np.empty(0, np.int64), np.arange(60)
        ra[6] = rb[6] = np.empty(0, np.int64)
        a = (np.concatenate(([0], np.cumsum([len(r) for r in ra]))), np.concatenate(ra))
        b = (np.concatenate(([0], np.cumsum([len(r) for r in rb]))), np.concatenate(rb))
    p, i = api._unite_rows(a, b)
    assert p.dtype == np.uint64 and i.dtype == np.uint64 and len(p) == m + 1 and int(p[0]) == 0 and int(p[-1]) == len(i)
    for r in range(m):
        assert np.array_equal(i[int(p[r]):int(p[r + 1])], np.union1d(ra[r], rb[r])), r
    # uint64 pairs whose row pointers do not start at 0 (a slice of a longer list) are read from their own start
    if m:
        shifted = (np.asarray(a[0], np.uint64) + np.uint64(3), np.concatenate((np.array([99, 98, 97], np.uint64), np.asarray(a[1], np.uint64))))
        p2, i2 = api._unite_rows(shifted, b)
        assert np.array_equal(p2, p) and np.array_equal(i2, i)
    with pytest.raises(ValueError):
        api._unite_rows(a, (np.zeros(m + 2, np.int64), np.empty(0, np.int64)))


# ---- 5. include=None is the call it was --------------------------------------------------------------------------------------------

class _Recorder:
    """stands in for the loaded library: notes the entry point a wrapper reached"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


def test_include_none_reaches_the_old_entry_points(monkeypatch):
    test, incl = ([0, 1, 2], [3, 4]), ([0, 2, 4], [3, 9, 4, 7])
    rec = _Recorder()
    s = _NoDeviceSession(True, rec)
    s.rank_batch([0, 1], test)
    s.rank_batch([0, 1], test, include=incl)
    s.eval_ranking(X_OK, exclude_seen=False)
    s.eval_ranking(X_OK, exclude_seen=False, include=_x([0, 1], [8, 2]))
    assert rec.calls == [("poismf_hip_session_rank_batch", 10), ("poismf_hip_session_rank_include", 12),
                         ("poismf_hip_session_rank_batch", 10), ("poismf_hip_session_rank_include", 12)]
    rec = _Recorder()
    monkeypatch.setattr(api, "load_library", lambda use_float: rec)
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    api.rank_batch(A, B, [0, 1], test)
    api.rank_batch(A, B, [0, 1], test, include=incl)
    _fake_fitted(True).eval_ranking(X_OK)
    _fake_fitted(True).eval_ranking(X_OK, include=_x([0, 1], [8, 2]))
    assert rec.calls == [("poismf_hip_rank_batch", 13), ("poismf_hip_rank_include", 15), ("poismf_hip_rank_batch", 13),
                         ("poismf_hip_rank_include", 15)]


def test_eval_ranking_unites_the_held_out_rows(monkeypatch):
    """what reaches the library: the negatives' rows with the users' held-out rows united in, strictly ascending"""
    seen = {}

    def fake(A, B, users, test, exclude=None, include=None):
        seen["include"] = include
        return np.zeros(len(test[1]), np.uint32), np.ones(len(users), np.uint32)

    monkeypatch.setattr(api, "rank_batch", fake)
    _fake_fitted(True).eval_ranking(X_OK, include=_x([0, 1, 1, 3], [8, 2, 9, 1]))      # users default to rows 0 and 1 of X_OK
    p, i = seen["include"]
    assert p.tolist() == [0, 2, 5] and i.tolist() == [5, 8, 2, 7, 9]
