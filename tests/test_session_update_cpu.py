"""Session updates without a device (include/poismf_hip.h section 2b): the header declares the entry points, built libraries export them,
and Session.add / Session.half_sweep_rows refuse bad arguments with ValueError before any library call -- checked on a Session object made
without a handle whose library is a stub that records every call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("poismf_hip_session_add_coo", "poismf_hip_session_get_matrix", "poismf_hip_half_sweep_rows")
DIMA, DIMB = 7, 5


class StubLib:
    """every attribute is a function that records its name and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def stub_session(use_float=True):
    s = object.__new__(api.Session)
    s.lib, s.h = StubLib(), None
    s.use_float, s.dimA, s.dimB, s.k = use_float, DIMA, DIMB, 4
    s.shardA, s.shardB = (0, DIMA), (0, DIMB)
    return s


def triplets(row, col, val, shape=(DIMA, DIMB)):
    """a COO-like object that, unlike scipy's, does not check its own indices"""
    return types.SimpleNamespace(row=np.asarray(row), col=np.asarray(col), data=np.asarray(val, dtype=np.float64), shape=shape)


def test_the_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "poismf_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"POISMF_HIP_API\s+int\s+" + name + r"\s*\(", text), name


def test_built_libraries_export_the_entry_points():
    for flavour in (False, True):
        path = build.lib_path(flavour)
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            for name in NAMES:
                assert hasattr(lib, name), (path, name)


def test_the_unit_is_registered():
    assert build.UNITS["session_update"] == ("session_update.hip", [])


def assert_the_unit_uses_the_shared_pieces(unit):
    """what the four units that change a resident matrix share has one home, session_merge.hpp: the eligibility rule, the two rocPRIM calls
    (scan_exclusive, touched_rows_on_device) and the owner of device scratch -- `unit` brings no second copy of any of them"""
    read = lambda name: open(os.path.join(build.CSRC, name)).read()
    shared, text = read("session_merge.hpp"), read(unit)
    assert re.search(r"^int eligible\(", shared, re.M) and "class Scratch" in shared
    assert "rocprim::exclusive_scan(" in shared and "rocprim::select(" in shared
    assert not re.search(r"^\s*(int|bool)\s+eligible\(", text, re.M), unit
    assert "eligible(s)" in text, unit   # ... and asks it
    assert "rocprim::exclusive_scan(" not in text and "rocprim::select(" not in text, unit
    assert not re.search(r"^\s*(?:virtual\s+)?~\w+\s*\(\s*\)", text, re.M), unit   # no struct with a destructor (that frees through pmf_free) of its own
    assert "whole_matrix_halves(" not in text and "while (0)" not in text, unit   # no inline copy of the rule, no do / while (0) ladder


def test_the_unit_uses_the_shared_pieces():
    assert_the_unit_uses_the_shared_pieces("session_update.hip")


BAD_UPDATES = {
    "wrong shape": triplets([0], [0], [1.0], shape=(DIMA, DIMB + 1)),
    "row == dimA": triplets([DIMA], [0], [1.0]),
    "col == dimB": triplets([0], [DIMB], [1.0]),
    "negative row": triplets([-1], [0], [1.0]),
    "value 0": triplets([0, 1], [0, 1], [1.0, 0.0]),
    "value -1": triplets([0, 1], [0, 1], [-1.0, 2.0]),
    "value nan": triplets([0], [0], [np.nan]),
    "value inf": triplets([0], [0], [np.inf]),
    "float indices": triplets([0.5], [0], [1.0]),
}


@pytest.mark.parametrize("use_float", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("what", list(BAD_UPDATES))
def test_add_refuses_before_any_library_call(what, use_float):
    s = stub_session(use_float)
    with pytest.raises(ValueError):
        s.add(BAD_UPDATES[what])
    assert s.lib.calls == []


def test_add_of_a_scipy_matrix_of_the_wrong_shape():
    s = stub_session()
    with pytest.raises(ValueError):
        s.add(sp.coo_matrix(([1.0], ([0], [0])), shape=(DIMA + 1, DIMB)))
    assert s.lib.calls == []


def test_add_of_an_empty_update_returns_0_without_a_library_call():
    s = stub_session()
    assert s.add(sp.coo_matrix((DIMA, DIMB))) == 0
    assert s.add(triplets([], [], [])) == 0
    assert s.lib.calls == []


def test_add_passes_a_good_update_on():
    s = stub_session()
    assert s.add(sp.coo_matrix(([1.0, 2.0], ([0, DIMA - 1], [DIMB - 1, 0])), shape=(DIMA, DIMB))) == 0   # (the stub reports no new cell)
    assert s.lib.calls == ["poismf_hip_session_add_coo"]


@pytest.mark.parametrize("which,dim", [(1, DIMA), (0, DIMB)])
@pytest.mark.parametrize("rows", ["[3, 3]", "[-1]", "[dim]", "[1.0, 2.0]", "[[1, 2]]"])
def test_half_sweep_rows_refuses_before_any_library_call(rows, which, dim):
    s = stub_session()
    with pytest.raises(ValueError):
        s.half_sweep_rows(which, eval(rows, {"dim": dim}), None, 1e-7, 1.0)
    assert s.lib.calls == []


def test_half_sweep_rows_of_no_rows_returns_0_without_a_library_call():
    s = stub_session()
    assert s.half_sweep_rows(1, [], None, 1e-7, 1.0) == 0
    assert s.half_sweep_rows(0, np.zeros(0, np.int64), None, 1e-7, 1.0, want_unchanged=True) == 0
    assert s.lib.calls == []
