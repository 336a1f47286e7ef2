"""New rows joining a resident session, without a device (include/poismf_hip.h section 2d): the header declares the entry points, built
libraries export them, the unit is registered, and Session.append / adopt_new / append_users / append_items refuse bad arguments with
ValueError before any library call -- checked on a Session object made without a handle whose library is a stub that records every call
(tests/test_session_update_cpu.py's pattern).  The Python object's dimensions and shards grow only when the library returned 0."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build
from tests.test_session_update_cpu import DIMA, DIMB, ROOT, assert_the_unit_uses_the_shared_pieces, stub_session

NAMES = ("poismf_hip_session_append_rows", "poismf_hip_session_adopt_new")
K = 4   # stub_session's


def test_the_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "poismf_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"POISMF_HIP_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in api.EXPORTED_SYMBOLS
    assert "2d. Session updates: the matrix grows" in text
    getters = text[text.index("Device pointers to the session-owned"):text.index("poismf_hip_session_factors_dirty(poismf_hip_session *s, int which);")]
    assert "DEAD" in getters and "2d" in getters   # (pointers obtained earlier do not survive a growth: said next to the getters)


def test_built_libraries_export_the_entry_points():
    for flavour in (False, True, "r"):
        path = build.lib_path(flavour)
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            for name in NAMES:
                assert hasattr(lib, name), (path, name)


def test_the_unit_is_registered():
    assert build.UNITS["session_grow"] == ("session_grow.hip", [])
    assert set(build.FLAVOURS) == {"d", "f", "r"}   # (every unit of UNITS is compiled for each)
    assert "session_merge.hpp" in build._deps("session_grow.hip")


def test_the_three_units_share_the_merge_through_the_header():
    """merge_half and its kernels live in session_merge.hpp once; session_grow.hip brings the growth kernels and no second scatter"""
    read = lambda name: open(os.path.join(build.CSRC, name)).read()
    kernels = lambda name: re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", read(name))
    shared = kernels("session_merge.hpp")
    assert "upd_scatter_kernel" in shared and "upd_place_kernel" in shared and "int merge_half(" in read("session_merge.hpp")
    for unit in ("session_update.hip", "session_remove.hip", "session_grow.hip"):
        assert not set(shared) & set(kernels(unit)), unit
        assert "int merge_half(" not in read(unit)
    assert set(kernels("session_grow.hip")) == {"grow_factor_kernel", "grow_indptr_kernel", "grow_major_kernel"}


def test_the_unit_uses_the_shared_pieces():
    assert_the_unit_uses_the_shared_pieces("session_grow.hip")


def rows_of(n, width, cells=((0, 0, 1.0),), dtype=np.float64):
    r, c, v = zip(*cells) if cells else ((), (), ())
    return sp.csr_matrix((np.array(v, dtype), (np.array(r, np.int64), np.array(c, np.int64))), shape=(n, width))


GOOD_USERS = rows_of(3, DIMB, ((0, 0, 1.0), (0, DIMB - 1, 2.0), (2, 1, 5.0)))
GOOD_ITEMS = rows_of(2, DIMA, ((1, DIMA - 1, 3.0),))
F_USERS, F_ITEMS = np.full((3, K), 0.5), np.full((2, K), 0.25)

# (which, X_new, factors, n_new)
BAD_APPENDS = {
    "users of the wrong width": (1, rows_of(3, DIMB + 1), None, None),
    "users of the items' width": (1, rows_of(3, DIMA), None, None),
    "items of the wrong width": (0, rows_of(2, DIMB), None, None),
    "a dense matrix": (1, np.ones((3, DIMB)), None, None),
    "factors with a row too few": (1, GOOD_USERS, np.ones((2, K)), None),
    "factors of the wrong k": (1, GOOD_USERS, np.ones((3, K + 1)), None),
    "one-dimensional factors": (1, GOOD_USERS, np.ones(3 * K), None),
    "factors with nan": (1, GOOD_USERS, np.where(np.eye(3, K) > 0, np.nan, 1.0), None),
    "factors with inf": (0, GOOD_ITEMS, np.full((2, K), np.inf), None),
    "empty rows with factors of another count": (1, None, np.ones((3, K)), 2),
    "value 0": (1, rows_of(3, DIMB, ((0, 0, 1.0), (1, 1, 0.0))), None, None),
    "value -1": (1, rows_of(3, DIMB, ((0, 0, -1.0),)), None, None),
    "value nan": (0, rows_of(2, DIMA, ((0, 0, np.nan),)), None, None),
    "value inf": (0, rows_of(2, DIMA, ((0, 0, np.inf),)), None, None),
    "duplicates that cancel": (1, sp.coo_matrix(([1.0, -1.0], ([0, 0], [2, 2])), shape=(3, DIMB)), None, None),
    "n_new against the matrix": (1, GOOD_USERS, None, 4),
    "nothing at all": (1, None, None, None),
    "a negative n_new": (1, None, None, -1),
    "a fractional n_new": (0, None, None, 1.5),
    "which 2": (2, GOOD_USERS, None, None),
    "which -1": (-1, GOOD_USERS, None, None),
    "which None": (None, GOOD_USERS, None, None),
    "which 'users'": ("users", GOOD_USERS, None, None),
    "which 0.5": (0.5, GOOD_USERS, None, None),
    "which True": (True, GOOD_USERS, None, None),
}


@pytest.mark.parametrize("use_float", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("what", list(BAD_APPENDS))
def test_append_refuses_before_any_library_call(what, use_float):
    s = stub_session(use_float)
    which, X_new, factors, n_new = BAD_APPENDS[what]
    with pytest.raises(ValueError):
        s.append(which, X_new, factors=factors, n_new=n_new)
    assert s.lib.calls == []
    assert (s.dimA, s.dimB, s.shardA, s.shardB) == (DIMA, DIMB, (0, DIMA), (0, DIMB))


def test_the_wrappers_refuse_before_any_library_call():
    s = stub_session()
    with pytest.raises(ValueError):
        s.append_users(rows_of(3, DIMB + 1), None, 3, factors=np.ones((3, K)))
    with pytest.raises(ValueError):
        s.append_users(rows_of(3, DIMB + 1), None, 3)                         # (before the fold-in, too)
    with pytest.raises(ValueError):
        s.append_users(rows_of(3, DIMB, ((0, 0, 0.0),)), None, 3)
    with pytest.raises(ValueError):
        s.append_items(rows_of(2, DIMA + 1), None, 1e-7, start=np.ones(K))
    with pytest.raises(ValueError):
        s.append_items(GOOD_ITEMS, None, 1e-7, start=np.ones(K + 1))
    with pytest.raises(ValueError):
        s.append_items(GOOD_ITEMS, None, 1e-7, start=np.full(K, np.nan))
    assert s.lib.calls == []
    assert (s.dimA, s.dimB) == (DIMA, DIMB)


def test_no_new_rows_return_the_dimension_without_a_library_call():
    s = stub_session()
    assert s.append(1, rows_of(0, DIMB, ())) == DIMA
    assert s.append(0, n_new=0) == DIMB
    assert s.append(1, factors=np.zeros((0, K))) == DIMA
    assert len(s.append_users(rows_of(0, DIMB, ()), None, 3)) == 0
    assert s.lib.calls == []
    assert (s.dimA, s.dimB, s.shardA, s.shardB) == (DIMA, DIMB, (0, DIMA), (0, DIMB))


@pytest.mark.parametrize("use_float", [True, False], ids=["f32", "f64"])
def test_good_calls_reach_exactly_their_entry_point(use_float):
    append = ["poismf_hip_session_append_rows"]
    for call, entry, grown in (
            (lambda s: s.append(1, GOOD_USERS), append, (DIMA + 3, DIMB)),
            (lambda s: s.append(1, GOOD_USERS.tocoo(), factors=F_USERS), append, (DIMA + 3, DIMB)),
            (lambda s: s.append(1, GOOD_USERS, n_new=3), append, (DIMA + 3, DIMB)),
            (lambda s: s.append(0, GOOD_ITEMS, factors=F_ITEMS.astype(np.float32)), append, (DIMA, DIMB + 2)),
            (lambda s: s.append(1, n_new=5), append, (DIMA + 5, DIMB)),
            (lambda s: s.append(0, n_new=np.int64(1), factors=np.ones((1, K))), append, (DIMA, DIMB + 1)),
            (lambda s: s.append(0, factors=F_ITEMS), append, (DIMA, DIMB + 2)),
            (lambda s: s.append_users(GOOD_USERS, None, 3, factors=F_USERS), append, (DIMA + 3, DIMB)),
            (lambda s: s.adopt_new(), ["poismf_hip_session_adopt_new"], (DIMA, DIMB)),   # (the stub reports no adopted row)
            (lambda s: s.append_items(GOOD_ITEMS, s.make_params("pg", 1e3), 1e-7, start=np.ones(K)),
             append + ["poismf_hip_half_sweep_rows"], (DIMA, DIMB + 2))):
        s = stub_session(use_float)
        s.lib.params_t = api._params_type(ctypes.c_float if use_float else ctypes.c_double)
        call(s)
        assert s.lib.calls == entry
        assert (s.dimA, s.dimB) == grown and s.shardA == (0, s.dimA) and s.shardB == (0, s.dimB)


def test_append_returns_the_first_new_row_and_the_wrappers_the_new_numbers():
    s = stub_session()
    assert s.append(1, GOOD_USERS) == DIMA and s.append(1, n_new=2) == DIMA + 3
    with pytest.raises(ValueError):
        s.append(0, GOOD_ITEMS)            # (the items' rows are as wide as the GROWN number of users now)
    assert s.append(0, rows_of(2, DIMA + 5)) == DIMB
    s = stub_session()
    assert np.array_equal(s.append_users(GOOD_USERS, None, 3, factors=F_USERS), np.arange(DIMA, DIMA + 3))


def test_append_users_without_factors_folds_in_and_adopts():
    s = stub_session()
    Bsum, Amean = np.ones(K), np.ones(K)
    p = api._params_type(ctypes.c_float)(1e3, 0., 1., 1e-7, 3, 1, 1, 0, 0)
    s.append_users(GOOD_USERS, p, 3, Bsum=Bsum, Amean=Amean)
    assert s.lib.calls == ["poismf_hip_session_factors_new", "poismf_hip_session_adopt_new"]


class Refusing:
    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return self.rc
        return fn


@pytest.mark.parametrize("rc,error", [(3, ValueError), (4, ValueError), (5, ValueError), (1, MemoryError)])
def test_the_library_s_return_codes_and_the_python_object_s_shape(rc, error):
    """rc 3 / 4 / 5 become ValueError, rc 1 MemoryError -- and the object keeps its dimensions and shards"""
    for call, entry in ((lambda s: s.append(1, GOOD_USERS, factors=F_USERS), "poismf_hip_session_append_rows"),
                        (lambda s: s.append(0, n_new=2), "poismf_hip_session_append_rows"),
                        (lambda s: s.append_users(GOOD_USERS, None, 3, factors=F_USERS), "poismf_hip_session_append_rows"),
                        (lambda s: s.append_items(GOOD_ITEMS, None, 1e-7, start=np.ones(K)), "poismf_hip_session_append_rows"),
                        (lambda s: s.adopt_new(), "poismf_hip_session_adopt_new")):
        s = stub_session()
        s.lib = Refusing(rc)
        with pytest.raises(error):
            call(s)
        assert s.lib.calls == [entry]
        assert (s.dimA, s.dimB, s.shardA, s.shardB) == (DIMA, DIMB, (0, DIMA), (0, DIMB))
