"""CPU-side checks of the batched top-N's boundary (include/poismf_hip.h section 1f): the header declares both prototypes with the
agreed parameter names and every library flavour exports them; PoisMF.topN_batch and Session.topn_batch's argument checks raise
before anything reaches a device; the C entry point itself answers 2 / 0 without one; and the one scratch allocation of a call
stays inside the budget the header states, for any number of users."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_topn_batch", "poismf_hip_session_topn_batch", "poismf_hip_topn_batch_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _params(name):
    text = open(HEADER).read()
    m = re.search(r"^POISMF_HIP_API\s+([\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, f"{name} is not declared"
    return " ".join(m.group(1).split()), [re.match(r".*?(\w+)$", " ".join(p.split())).group(1) for p in m.group(2).split(",")]


def _define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1))


def test_header_declares_the_prototypes():
    ret, names = _params("poismf_hip_session_topn_batch")
    assert ret == "int"
    assert names == ["s", "users", "n_users", "n_top", "exclude_seen", "excl_indptr", "excl_indices", "out_ix", "out_score"]
    ret, names = _params("poismf_hip_topn_batch")
    assert ret == "int"
    assert names == ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "excl_indptr", "excl_indices", "out_ix", "out_score"]
    ret, names = _params("poismf_hip_topn_batch_scratch_bytes")
    assert ret == "size_t" and names == ["n_users", "n_top", "dimB", "k"]
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_TOPN_BATCH_MAX_N_TOP") >= 128
    assert _define("POISMF_HIP_TOPN_BATCH_MAX_N_TOP") == api.TOPN_BATCH_MAX_N_TOP


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_batch(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def test_topn_batch_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_batch([0, 1])


NUSERS, NITEMS, K = 6, 300, 3


def _fake_fitted(use_float):
    """a model that looks fitted without any fit having run (no device is touched)"""
    m = api.PoisMF(k=K, use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    m.nusers, m.nitems = NUSERS, NITEMS
    m.is_fitted = True
    return m


# (users, n, exclude as (indptr, indices) or None): every one invalid
BAD = {
    "user-out-of-range": ([0, NUSERS], 5, None),
    "negative-user": ([-1, 0], 5, None),
    "item-out-of-range": ([0, 1], 5, ([0, 1, 2], [3, NITEMS])),
    "negative-item": ([0, 1], 5, ([0, 1, 2], [-2, 4])),
    "descending-row": ([0, 1], 5, ([0, 2, 4], [1, 2, 9, 7])),
    "repeated-item": ([0, 1], 5, ([0, 2, 4], [1, 2, 7, 7])),
    "n-zero": ([0, 1], 0, None),
    "n-above-items-left": ([0, 1], 100, ([0, 0, 201], list(range(201)))),
    "n-above-limit": ([0, 1], 129, None),
    "exclude-wrong-rows": ([0, 1], 5, ([0, 1, 2, 3], [1, 2, 3])),
}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_batch(users, n, exclude=excl)


def test_scipy_exclude_with_wrong_row_count_raises():
    X = sp.csr_matrix((np.ones(3), (np.array([0, 1, 2]), np.array([1, 2, 3]))), shape=(3, NITEMS))
    with pytest.raises(ValueError):
        _fake_fitted(True).topN_batch([0, 1], 5, exclude=X)


def _with_stored_zero():
    """two rows of `exclude`, out of order, with a repeated cell and a stored zero: row 0 = {7, 2 (twice), 5 (value 0)}, row 1 = {9}"""
    data = np.array([1.0, 1.0, 1.0, 0.0, 1.0])
    cols = np.array([7, 2, 2, 5, 9])
    return sp.csr_matrix((data, cols, np.array([0, 4, 5])), shape=(2, NITEMS))


def test_topn_exclude_takes_what_csr_matrix_takes_and_keeps_stored_zeros():
    """the top-N side of `exclude`: anything scipy.sparse.csr_matrix() accepts; duplicates merged, rows sorted, and a cell stored
    with the value zero stays excluded"""
    X = _with_stored_zero()
    _, indptr, indices = api._topn_batch_args([0, 1], 5, X, NUSERS, NITEMS)
    assert indptr.dtype == np.uint64 and indices.dtype == np.uint64
    assert indptr.tolist() == [0, 3, 4] and indices.tolist() == [2, 5, 7, 9]
    dense = np.zeros((2, NITEMS))
    dense[0, [7, 2]] = 1.0
    dense[1, 9] = 3.0
    _, indptr, indices = api._topn_batch_args([0, 1], 5, dense, NUSERS, NITEMS)
    assert indptr.tolist() == [0, 2, 3] and indices.tolist() == [2, 7, 9]
    with pytest.raises(ValueError):   # the row count still counts
        api._topn_batch_args([0, 1, 2], 5, dense, NUSERS, NITEMS)


def test_rank_lists_need_a_sparse_matrix_or_a_pair_and_drop_stored_zeros():
    """the rank side of the same argument: a dense array is refused, and a cell stored with the value zero is no cell"""
    X = _with_stored_zero()
    _, tp, ti, ep, ei = api._rank_batch_args([0, 1], X, X, NUSERS, NITEMS, K)
    assert tp.tolist() == [0, 2, 3] and ti.tolist() == [2, 7, 9]
    assert ep.tolist() == [0, 2, 3] and ei.tolist() == [2, 7, 9]
    dense = np.zeros((2, NITEMS))
    dense[0, 7] = 1.0
    with pytest.raises(ValueError, match="must be a SciPy sparse matrix"):
        api._rank_batch_args([0, 1], dense, None, NUSERS, NITEMS, K)
    with pytest.raises(ValueError, match="must be a SciPy sparse matrix"):
        api._rank_batch_args([0, 1], X, dense, NUSERS, NITEMS, K)


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self, use_float):
        self.lib = None
        self.use_float = use_float
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, 4), (0, NITEMS)
        self.h = None


@pytest.mark.parametrize("case", sorted(BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_batch(users, n, exclude=excl)


def test_session_wrapper_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_batch([1, 5], 5, exclude_seen=True)


def _c_call(flavour, users, n, excl, n_users=None):
    """poismf_hip_topn_batch itself through ctypes; index arrays in the flavour's sparse_ix"""
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
    rc = lib.poismf_hip_topn_batch(p(A), p(B), K, NUSERS, NITEMS, p(u), m, n, p(ip) if ip is not None else None,
                                   p(ii) if ii is not None else None, p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))   # (a C caller has no row count to get wrong)
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, n, excl = BAD[case]
    rc, out, sc = _c_call(flavour, users, n, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, sc = _c_call(flavour, [0], 5, None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_call(flavour, [0], 0, None, n_users=0)   # (not even n_top = 0 matters then)
    assert rc == 0


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u = np.zeros(1, np.uint64)
    out = np.zeros(1, np.uint64)
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_batch(api._ptr(A), api._ptr(A), k, 2, 2, api._ptr(u), 1, 1, None, None, api._ptr(out), None) == 2


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_stated_budget(flavour):
    """the size both entry points allocate (one allocation per call), against the figure in the header's own text"""
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    limit = _define("POISMF_HIP_TOPN_BATCH_MAX_N_TOP")
    fn = api.load_library(flavour).poismf_hip_topn_batch_scratch_bytes
    kmax = 512 if flavour else 256
    users = sorted({1, 2, 63, 64, 65, 1000, 4096, 10 ** 5, 10 ** 6, 10 ** 7} | {int(x) for x in np.logspace(0, 7, 40)})
    tops = sorted({1, 2, 10, 16, 17, 64, 100, limit - 1, limit})
    items = sorted({1, 2, 64, 1000, 25000, 10 ** 5, 10 ** 6, 2 ** 31 - 1})
    worst = 0
    for m in users:
        for n in tops:
            for dimB in items:
                for k in (1, 50, kmax):
                    b = int(fn(m, n, dimB, k))
                    assert 0 < b <= budget, (m, n, dimB, k, b)
                    worst = max(worst, b)
    # a small call does not pay for a large one
    assert int(fn(64, 10, 1000, 50)) < (8 << 20)
    assert worst > (budget >> 2)   # (the bound is not vacuous: large calls do use a good part of it)
