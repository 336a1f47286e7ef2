"""CPU-side checks of the fold-in boundary (include/poismf_hip.h section 1m, new rows against a resident B): the header declares the
four prototypes with the agreed parameter names and every library flavour exports them; the host-pointer entry answers 2 with
nothing written -- and 0 for no rows -- before any device is looked for, and so do the session entries as far as they can be
called without a session; PoisMF.topN_new and Session.transform / topn_new / rank_new / eval_ranking_new raise on bad arguments
before anything reaches a device.  (What the session entries refuse on a live session is in tests/test_gpu_fold_in.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_session_factors_new", "poismf_hip_session_topn_new", "poismf_hip_session_rank_new", "poismf_hip_topn_new")
ROWS = ["Xr", "Xr_indptr", "Xr_indices", "n_new", "Bsum", "Amean", "p", "niter"]
EXCL = ["exclude_own", "excl_indptr", "excl_indices"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _params(name):
    text = open(HEADER).read()
    m = re.search(r"^POISMF_HIP_API\s+([\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, f"{name} is not declared"
    return " ".join(m.group(1).split()), [re.match(r".*?(\w+)$", " ".join(p.split())).group(1) for p in m.group(2).split(",")]


def test_header_declares_the_prototypes():
    assert _params("poismf_hip_session_factors_new") == ("int", ["s"] + ROWS + ["out_A"])
    assert _params("poismf_hip_session_topn_new") == ("int", ["s"] + ROWS + ["n_top"] + EXCL + ["out_ix", "out_score", "out_A"])
    assert _params("poismf_hip_session_rank_new") == ("int", ["s"] + ROWS + ["test_indptr", "test_indices"] + EXCL +
                                                      ["out_rank", "out_n_adm", "out_A"])
    assert _params("poismf_hip_topn_new") == ("int", ["B", "Bsum", "Amean", "Xr", "Xr_indptr", "Xr_indices", "k", "dimB", "n_new", "l2_reg",
                                                      "w_mult", "step_size", "niter", "maxupd", "method", "limit_step", "reuse_mean", "n_top"] +
                                              EXCL + ["out_ix", "out_score", "out_A"])
    assert "1m. New rows against a resident B" in open(HEADER).read()
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_the_entries(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def test_the_unit_is_in_the_build_table():
    assert build.UNITS["fold_in"] == ("fold_in.hip", [])
    assert {"session.hpp", "tb_batch.hpp"} <= set(build._deps("fold_in.hip"))


NITEMS, K = 300, 3
ROWS2 = ([0, 2, 3], [4, 9, 7])          # two valid new rows: {4, 9} and {7}

# (new rows as (indptr, indices), n_top, exclude_own, exclude as (indptr, indices) or None): every one invalid
BAD = {
    "item-out-of-range": (([0, 2, 3], [4, NITEMS, 7]), 5, 1, None),
    "negative-item": (([0, 2, 3], [4, -3, 7]), 5, 1, None),
    "row-pointers-decrease": (([0, 2, 1], [4, 9, 7]), 5, 1, None),
    "negative-row-pointer": (([-1, 2, 3], [4, 9, 7]), 5, 1, None),
    "n-zero": (ROWS2, 0, 1, None),
    "n-above-limit": (ROWS2, 129, 1, None),
    "n-above-items": (ROWS2, NITEMS + 1, 0, None),
    "n-above-items-left-by-list": (ROWS2, 100, 0, ([0, 0, 201], list(range(201)))),
    "n-above-items-left-with-own-row": (([0, 2, 3], [250, 260, 7]), 100, 1, ([0, 199, 199], list(range(199)))),
    "exclude-item-out-of-range": (ROWS2, 5, 1, ([0, 1, 2], [3, NITEMS])),
    "exclude-row-descending": (ROWS2, 5, 1, ([0, 2, 4], [1, 2, 9, 7])),
    "exclude-row-repeats": (ROWS2, 5, 0, ([0, 2, 4], [1, 2, 7, 7])),
}


def _ix(flavour, a):
    a = np.asarray(a, np.int64)
    return a.astype(np.int32) if flavour == "r" else a.view(np.uint64).copy()


def _c_call(flavour, rows, n, own, excl, n_new=None, k=K, null=()):
    """poismf_hip_topn_new itself through ctypes, index arrays in the flavour's sparse_ix; outputs filled with sentinels"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64
    B, Bsum, Amean = np.ones((NITEMS, K), dt), np.full(K, float(NITEMS), dt), np.ones(K, dt)
    ip, ii = _ix(flavour, rows[0]), _ix(flavour, rows[1])
    X = np.ones(len(ii), dt)
    m = len(ip) - 1 if n_new is None else n_new
    out = np.full((max(m, 1), max(n, 1)), 12345, it)
    sc = np.full((max(m, 1), max(n, 1)), -7.0, dt)
    fac = np.full((max(m, 1), K), -7.0, dt)
    p = api._ptr
    ep, ei = (_ix(flavour, excl[0]), _ix(flavour, excl[1])) if excl is not None else (None, None)
    arg = dict(B=p(B), Bsum=p(Bsum), Amean=p(Amean), Xr=p(X), out_ix=p(out))
    arg.update({name: None for name in null})
    rc = lib.poismf_hip_topn_new(arg["B"], arg["Bsum"], arg["Amean"], arg["Xr"], p(ip), p(ii), k, NITEMS, m, 1e9, 1.0, 1e-7, 10, 1, 3, True, False,
                                 n, own, p(ep) if ep is not None else None, p(ei) if ei is not None else None, arg["out_ix"], p(sc), p(fac))
    return rc, out, sc, fac


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    rows, n, own, excl = BAD[case]
    rc, out, sc, fac = _c_call(flavour, rows, n, own, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0) and np.all(fac == -7.0)


@pytest.mark.parametrize("null", ["B", "Bsum", "Amean", "Xr", "out_ix"])
def test_c_entry_null_pointers(null):
    rc, out, sc, fac = _c_call(True, ROWS2, 5, 1, None, null=(null,))
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0) and np.all(fac == -7.0)


def test_c_entry_k_out_of_range():
    for k in (0, -1, 513):
        rc, out, sc, fac = _c_call(True, ROWS2, 5, 1, None, k=k)
        assert rc == 2 and np.all(out == 12345) and np.all(fac == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_rows_is_not_an_error(flavour):
    rc, out, sc, fac = _c_call(flavour, ([0], []), 5, 1, None, n_new=0)
    assert rc == 0 and np.all(out == 12345) and np.all(sc == -7.0) and np.all(fac == -7.0)
    rc, _, _, _ = _c_call(flavour, ([0], []), 0, 1, None, n_new=0)   # (not even n_top = 0 matters then)
    assert rc == 0


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_session_entries_without_a_session(flavour):
    """no rows: 0 whatever else is passed; rows and no session: 2, nothing written"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64
    ip, ii, X = _ix(flavour, ROWS2[0]), _ix(flavour, ROWS2[1]), np.ones(3, dt)
    Bsum, Amean = np.full(K, 300.0, dt), np.ones(K, dt)
    par = lib.params_t(1e9, 0.0, 1.0, 1e-7, 3, 1, 1, 0, 0)
    out, sc, fac = np.full((2, 5), 12345, it), np.full((2, 5), -7.0, dt), np.full((2, K), -7.0, dt)
    rk, na = np.full(3, 12345, np.uint32), np.full(2, 12345, np.uint32)
    p = api._ptr
    for m, want in ((0, 0), (2, 2)):
        lead = [None, p(X), p(ip), p(ii), m, p(Bsum), p(Amean), C.byref(par), 10]
        assert lib.poismf_hip_session_factors_new(*lead, p(fac)) == want
        assert lib.poismf_hip_session_topn_new(*lead, 5, 1, None, None, p(out), p(sc), p(fac)) == want
        assert lib.poismf_hip_session_rank_new(*lead, p(ip), p(ii), 1, None, None, p(rk), p(na), p(fac)) == want
        assert np.all(out == 12345) and np.all(sc == -7.0) and np.all(fac == -7.0) and np.all(rk == 12345) and np.all(na == 12345)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _X(rows=2, cols=NITEMS):
    return sp.csr_matrix((np.ones(3), np.array([4, 9, 7]), np.array([0, 2, 3] + [3] * (rows - 2))), shape=(rows, cols))


def _X_bad_index():
    X = _X()
    X.indices = np.array([4, NITEMS + 5, 7], X.indices.dtype)   # (SciPy does not look at the indices of a matrix that exists)
    return X


def _fake_fitted(use_float=True):
    """a model that looks fitted without any fit having run (no device is touched)"""
    m = api.PoisMF(k=K, method="pg", use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((6, K), dt), np.ones((NITEMS, K), dt)
    m.nusers, m.nitems = 6, NITEMS
    m.Bsum, m.Amean = m.B.sum(axis=0), m.A.mean(axis=0)
    m.is_fitted = True
    return m


class _NoDeviceSession(api.Session):
    """the session wrapper's argument checks without a session behind it"""

    def __init__(self, use_float, shardA=(0, 6)):
        self.lib = api.load_library(use_float)
        self.use_float = use_float
        self.dimA, self.dimB, self.k = 6, NITEMS, K
        self.shardA, self.shardB = shardA, (0, NITEMS)
        self.h = None


STATS = dict(Bsum=np.full(K, 300.0), Amean=np.ones(K))

# (X_new, top_n, exclude): every one invalid
BAD_PY = {
    "wrong-column-count": (lambda: _X(cols=NITEMS - 1), 5, None),
    "dense-rows": (lambda: np.ones((2, NITEMS)), 5, None),
    "index-out-of-range": (_X_bad_index, 5, None),
    "n-above-limit": (_X, 129, None),
    "n-zero": (_X, 0, None),
    "exclude-wrong-rows": (_X, 5, ([0, 1, 2, 3], [1, 2, 3])),
    "exclude-scipy-wrong-rows": (_X, 5, _X(rows=3)),
    "n-above-items-left": (_X, 100, ([0, 0, 201], list(range(201)))),
}


def test_topn_new_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_new(_X())


@pytest.mark.parametrize("case", sorted(BAD_PY))
def test_invalid_input_raises_before_the_device(case):
    X, n, excl = BAD_PY[case]
    with pytest.raises(ValueError):
        _fake_fitted().topN_new(X(), n, exclude=excl)
    s = _NoDeviceSession(True)
    par = s.make_params("pg", 1e9)
    with pytest.raises(ValueError):
        s.topn_new(X(), par, 10, top_n=n, exclude=excl, **STATS)


@pytest.mark.parametrize("case", ["wrong-column-count", "dense-rows", "index-out-of-range"])
def test_every_session_call_checks_the_rows(case):
    X = BAD_PY[case][0]
    s = _NoDeviceSession(False)
    par = s.make_params("cg", 1e4)
    test = ([0, 1, 2], [5, 6])
    with pytest.raises(ValueError):
        s.transform(X(), par, 10, **STATS)
    with pytest.raises(ValueError):
        s.rank_new(X(), test, par, 10, **STATS)
    with pytest.raises(ValueError):
        s.eval_ranking_new(X(), _X(), par, 10, **STATS)


def test_rank_new_checks_its_lists():
    s = _NoDeviceSession(True)
    par = s.make_params("pg", 1e9)
    for test, excl in ((([0, 1, 2, 3], [5, 6, 7]), None),             # a row too many
                       (([0, 2, 2], [6, 5]), None),                   # a descending held-out row
                       (([0, 1, 2], [5, NITEMS]), None),              # an item out of range
                       (([0, 1, 2], [5, 6]), ([0, 1], [3]))):         # an exclusion row too few
        with pytest.raises(ValueError):
            s.rank_new(_X(), test, par, 10, exclude=excl, **STATS)
    with pytest.raises(ValueError):
        s.eval_ranking_new(_X(), _X(rows=3), par, 10, **STATS)        # held-out rows of another shape
    with pytest.raises(ValueError):
        s.eval_ranking_new(_X(), _X(), par, 10, k=0, **STATS)


def test_stats_must_have_k_entries():
    s = _NoDeviceSession(True)
    with pytest.raises(ValueError, match="k = 3"):
        s.transform(_X(), s.make_params("pg", 1e9), 10, Bsum=np.ones(K + 1), Amean=np.ones(K))


@pytest.mark.parametrize("given", [{}, {"Bsum": np.ones(K)}, {"Amean": np.ones(K)}])
def test_a_shard_only_session_asks_for_the_stats(given):
    s = _NoDeviceSession(True, shardA=(0, 4))
    par = s.make_params("pg", 1e9)
    with pytest.raises(ValueError, match="Bsum and Amean"):
        s.transform(_X(), par, 10, **given)
    with pytest.raises(ValueError, match="Bsum and Amean"):
        s.topn_new(_X(), par, 10, **given)


def test_the_rows_are_coerced_as_transform_coerces_them():
    """COO with a repeated cell and unsorted columns -> CSR, duplicates summed, indices sorted, the flavour's types"""
    coo = sp.coo_matrix((np.array([1.0, 2.0, 3.0, 4.0]), (np.array([1, 0, 1, 1]), np.array([9, 4, 2, 9]))), shape=(3, NITEMS))
    data, indptr, indices = api._new_rows_args(coo, NITEMS, True)
    assert data.dtype == np.float32 and indptr.dtype == np.uint64 and indices.dtype == np.uint64
    assert indptr.tolist() == [0, 1, 3, 3] and indices.tolist() == [4, 2, 9] and data.tolist() == [2.0, 3.0, 5.0]
