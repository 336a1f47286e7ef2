"""Counts taken back from a resident session, without a device (include/poismf_hip.h section 2c): the header declares the entry points, built
libraries export them, the unit is registered, and Session.subtract / remove / forget / retract refuse bad arguments with ValueError before any
library call -- checked on a Session object made without a handle whose library is a stub that records every call
(tests/test_session_update_cpu.py's pattern)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build
from tests.test_session_update_cpu import DIMA, DIMB, ROOT, assert_the_unit_uses_the_shared_pieces, stub_session, triplets

NAMES = ("poismf_hip_session_sub_coo", "poismf_hip_session_remove_rows")


def test_the_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "poismf_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"POISMF_HIP_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in api.EXPORTED_SYMBOLS
    assert "2c. Session updates: counts are taken back" in text


def test_built_libraries_export_the_entry_points():
    for flavour in (False, True):
        path = build.lib_path(flavour)
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            for name in NAMES:
                assert hasattr(lib, name), (path, name)


def test_the_unit_is_registered():
    assert build.UNITS["session_remove"] == ("session_remove.hip", [])
    assert build.UNITS["session_update"] == ("session_update.hip", [])
    assert "session_merge.hpp" in build._deps("session_remove.hip") and "session_merge.hpp" in build._deps("session_update.hip")


def test_the_two_units_share_their_kernels_through_the_header():
    """no kernel of session_merge.hpp is defined a second time in either unit"""
    read = lambda name: open(os.path.join(build.CSRC, name)).read()
    shared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", read("session_merge.hpp"))
    assert "upd_locate_kernel" in shared
    for unit in ("session_update.hip", "session_remove.hip"):
        defined = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", read(unit))
        assert not set(shared) & set(defined), unit
    assert "rem_compact_kernel" in re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", read("session_remove.hip"))


def test_the_unit_uses_the_shared_pieces():
    assert_the_unit_uses_the_shared_pieces("session_remove.hip")


BAD_CELLS = {
    "wrong shape": triplets([0], [0], [1.0], shape=(DIMA, DIMB + 1)),
    "row == dimA": triplets([DIMA], [0], [1.0]),
    "col == dimB": triplets([0], [DIMB], [1.0]),
    "negative row": triplets([-1], [0], [1.0]),
    "float indices": triplets([0.5], [0], [1.0]),
    "two-dimensional lengths differ": triplets([0, 1], [0], [1.0, 1.0]),
}
BAD_VALUES = {
    "value 0": triplets([0, 1], [0, 1], [1.0, 0.0]),
    "value -1": triplets([0, 1], [0, 1], [-1.0, 2.0]),
    "value nan": triplets([0], [0], [np.nan]),
    "value inf": triplets([0], [0], [np.inf]),
}
GOOD = sp.coo_matrix(([1.0, 2.0], ([0, DIMA - 1], [DIMB - 1, 0])), shape=(DIMA, DIMB))


@pytest.mark.parametrize("use_float", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("what", list(BAD_CELLS) + list(BAD_VALUES))
def test_subtract_refuses_before_any_library_call(what, use_float):
    s = stub_session(use_float)
    for missing in ("raise", "ignore"):
        with pytest.raises(ValueError):
            s.subtract({**BAD_CELLS, **BAD_VALUES}[what], missing=missing)
    assert s.lib.calls == []


@pytest.mark.parametrize("what", list(BAD_CELLS))
def test_remove_refuses_before_any_library_call(what):
    s = stub_session()
    with pytest.raises(ValueError):
        s.remove(BAD_CELLS[what])
    assert s.lib.calls == []


@pytest.mark.parametrize("what", list(BAD_VALUES))
def test_remove_does_not_read_the_values(what):
    s = stub_session()
    assert s.remove(BAD_VALUES[what]) == 0   # (the stub reports no removed cell)
    assert s.lib.calls == ["poismf_hip_session_sub_coo"]
    no_data = lambda: None
    no_data.row, no_data.col, no_data.shape = np.array([1, 2]), np.array([0, 0]), (DIMA, DIMB)
    assert s.remove(no_data) == 0
    assert s.lib.calls == ["poismf_hip_session_sub_coo"] * 2


@pytest.mark.parametrize("method", ["subtract", "remove"])
@pytest.mark.parametrize("missing", ["skip", None, True, "RAISE", ""])
def test_missing_must_be_one_of_the_two_words(method, missing):
    s = stub_session()
    with pytest.raises(ValueError):
        getattr(s, method)(GOOD, missing=missing)
    assert s.lib.calls == []


def test_a_scipy_matrix_of_the_wrong_shape():
    s = stub_session()
    for method in (s.subtract, s.remove):
        with pytest.raises(ValueError):
            method(sp.coo_matrix(([1.0], ([0], [0])), shape=(DIMA + 1, DIMB)))
    with pytest.raises(ValueError):
        s.retract(sp.coo_matrix(([1.0], ([0], [0])), shape=(DIMA + 1, DIMB)), None, 1e-7)
    assert s.lib.calls == []


def test_empty_inputs_return_0_without_a_library_call():
    s = stub_session()
    for method in (s.subtract, s.remove):
        assert method(sp.coo_matrix((DIMA, DIMB))) == 0
        assert method(triplets([], [], [])) == 0
    assert s.forget(1, []) == 0
    assert s.forget(0, np.zeros(0, np.int64)) == 0
    assert s.lib.calls == []


def test_good_calls_reach_exactly_their_entry_point():
    for call, entry in ((lambda s: s.subtract(GOOD), "poismf_hip_session_sub_coo"),
                        (lambda s: s.subtract(GOOD, missing="ignore"), "poismf_hip_session_sub_coo"),
                        (lambda s: s.remove(GOOD), "poismf_hip_session_sub_coo"),
                        (lambda s: s.remove(GOOD.tocsr(), missing="raise"), "poismf_hip_session_sub_coo"),
                        (lambda s: s.forget(1, [DIMA - 1, 0]), "poismf_hip_session_remove_rows"),
                        (lambda s: s.forget(0, np.array([DIMB - 1], np.int32)), "poismf_hip_session_remove_rows")):
        s = stub_session()
        assert call(s) == 0   # (the stub reports no removed cell)
        assert s.lib.calls == [entry]


@pytest.mark.parametrize("which,dim", [(1, DIMA), (0, DIMB)])
@pytest.mark.parametrize("rows", ["[3, 3]", "[-1]", "[dim]", "[1.0, 2.0]", "[[1, 2]]", "[True, False]"])
def test_forget_refuses_before_any_library_call(rows, which, dim):
    s = stub_session()
    with pytest.raises(ValueError):
        s.forget(which, eval(rows, {"dim": dim}))
    assert s.lib.calls == []


@pytest.mark.parametrize("which", [2, -1, None, "users", 0.5])
def test_forget_wants_which_0_or_1(which):
    s = stub_session()
    with pytest.raises(ValueError):
        s.forget(which, [0])
    assert s.lib.calls == []


def test_the_library_s_refusals_become_value_errors():
    class Refusing:
        def __init__(self, rc):
            self.rc, self.calls = rc, []

        def __getattr__(self, name):
            def fn(*args):
                self.calls.append(name)
                return self.rc
            return fn

    for rc in (3, 4, 5, 6):
        s = stub_session()
        s.lib = Refusing(rc)
        with pytest.raises(ValueError):
            s.subtract(GOOD)
        with pytest.raises(ValueError):
            s.remove(GOOD)
        if rc in (3, 5):
            with pytest.raises(ValueError):
                s.forget(1, [0])
    s = stub_session()
    s.lib = Refusing(1)
    with pytest.raises(MemoryError):
        s.subtract(GOOD)
    with pytest.raises(MemoryError):
        s.forget(0, [0])


@pytest.mark.parametrize("use_float", [True, False], ids=["f32", "f64"])
def test_add_still_refuses_0_and_minus_1(use_float):
    s = stub_session(use_float)
    for v in (0.0, -1.0):
        with pytest.raises(ValueError):
            s.add(triplets([0, 1], [0, 1], [1.0, v]))
    assert s.lib.calls == []
