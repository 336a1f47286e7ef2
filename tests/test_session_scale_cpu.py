"""Session.decay / poismf_hip_session_scale (include/poismf_hip.h section 2e) without a GPU: the header, the export list, the build unit,
the binding's refusals before any library call (tests/test_session_update_cpu.py's stub session), the mapping of the return codes, and
the numpy expectation of tests/session_scale_values.py checked against cases worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build
from tests.session_scale_values import expected
from tests.test_session_update_cpu import DIMA, DIMB, assert_the_unit_uses_the_shared_pieces, stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "poismf_hip_session_scale"


def test_the_header_declares_the_entry_point():
    with open(os.path.join(ROOT, "include", "poismf_hip.h")) as fh:
        text = fh.read()
    assert re.search(r"POISMF_HIP_API\s+int\s+" + NAME + r"\s*\(", text)
    assert re.search(r"^ \* 2e\. ", text, re.M)
    assert text.index(" * 2d. ") < text.index(" * 2e. ") < text.index(NAME)
    assert NAME in api.EXPORTED_SYMBOLS


def test_built_libraries_export_the_entry_point():
    for flavour in (False, True, "r"):
        path = build.lib_path(flavour)
        if os.path.exists(path):
            assert hasattr(ctypes.CDLL(path), NAME), path


def test_the_unit_is_registered_and_brings_kernels_of_its_own():
    assert build.UNITS["session_scale"] == ("session_scale.hip", [])
    assert "session_merge.hpp" in build._deps("session_scale.hip")
    read = lambda name: open(os.path.join(build.CSRC, name)).read()
    kernels = lambda name: re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", read(name))
    shared, own = kernels("session_merge.hpp"), kernels("session_scale.hip")
    assert "upd_scatter_kernel" in shared and not set(shared) & set(own)
    assert set(own) == {"scl_decide_kernel", "scl_indptr_kernel", "scl_compact_kernel", "scl_inplace_kernel"}


def test_the_unit_uses_the_shared_pieces():
    assert_the_unit_uses_the_shared_pieces("session_scale.hip")


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
class RecordingLib:
    """every attribute is a function that records its name and arguments and returns `rc`; what the two vector arguments of the entry
    point point to is copied while the call runs (the arrays are the binding's own)"""

    def __init__(self, rc, ctype):
        self.calls, self.vectors, self.rc, self.ctype = [], [], rc, ctype

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == NAME:
                peek = lambda p, n: None if p is None else np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(self.ctype)), (n,)).copy()
                self.vectors.append((peek(args[2], DIMA), peek(args[3], DIMB)))
            return self.rc
        return fn


def recording_session(use_float, rc=0):
    s = stub_session(use_float)
    s.lib = RecordingLib(rc, ctypes.c_float if use_float else ctypes.c_double)
    return s


BAD_SCALARS = (-1.0, np.nan, np.inf)
BAD_CALLS = {}
for v in BAD_SCALARS:
    BAD_CALLS[f"gamma {v}"] = dict(gamma=v)
    BAD_CALLS[f"floor {v}"] = dict(floor=v)
    for name, dim in (("users", DIMA), ("items", DIMB)):
        vec = np.ones(dim)
        vec[dim // 2] = v
        BAD_CALLS[f"{name} holds {v}"] = {name: vec}
for name, dim in (("users", DIMA), ("items", DIMB)):
    BAD_CALLS[f"{name} one short"] = {name: np.ones(dim - 1)}
    BAD_CALLS[f"{name} one long"] = {name: np.ones(dim + 1)}
    BAD_CALLS[f"{name} two-dimensional"] = {name: np.ones((dim, 1))}
    BAD_CALLS[f"{name} boolean"] = {name: np.ones(dim, bool)}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("what", sorted(BAD_CALLS))
def test_decay_refuses_before_any_library_call(what, use_float):
    s = recording_session(use_float)
    with pytest.raises(ValueError, match="decay"):
        s.decay(**BAD_CALLS[what])
    assert s.lib.calls == []


def test_a_gamma_beyond_the_session_s_precision_is_refused():
    s = recording_session(True)
    with pytest.raises(ValueError), np.errstate(over="ignore"):
        s.decay(1e39)           # infinite as a float32
    assert s.lib.calls == []
    recording_session(False).decay(1e39)


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
def test_a_good_call_reaches_the_entry_point(use_float):
    dt = np.float32 if use_float else np.float64
    s = recording_session(use_float)
    assert s.decay(0.9) == 0
    assert s.decay(0.5, floor=0.25, users=np.linspace(0, 1, DIMA), items=[2] * DIMB) == 0
    assert s.decay(users=np.arange(DIMA)) == 0 and s.decay(items=np.arange(DIMB, dtype=np.int32)) == 0
    assert [name for name, _ in s.lib.calls] == [NAME] * 4
    (_, a), (_, b), (_, c), (_, d) = s.lib.calls
    assert a[1] == float(dt(0.9)) and a[2] is None and a[3] is None and a[4] == 0.0
    assert b[1] == 0.5 and b[4] == 0.25 and b[2] is not None and b[3] is not None
    users, items = s.lib.vectors[1]
    assert users.dtype == dt and np.array_equal(users, np.linspace(0, 1, DIMA).astype(dt))      # converted to the session's dtype
    assert np.array_equal(items, np.full(DIMB, 2, dt))
    assert c[2] is not None and c[3] is None and d[2] is None and d[3] is not None
    assert np.array_equal(s.lib.vectors[3][1], np.arange(DIMB, dtype=dt))


@pytest.mark.parametrize("rc, exc", [(4, ValueError), (5, ValueError), (7, ValueError), (1, MemoryError), (2, MemoryError)])
def test_return_codes(rc, exc):
    s = recording_session(True, rc)
    with pytest.raises(exc) as e:
        s.decay(0.5)
    assert len(s.lib.calls) == 1
    if rc == 7:
        assert "a scaled value is not finite; nothing was changed" in str(e.value)


# ---- the expectation, by hand ----------------------------------------------------------------------------------------------------------
PREC = pytest.mark.parametrize("prec", [False, True], ids=["f64", "f32"])


@PREC
def test_expected_on_three_by_three(prec):
    X = sp.csr_matrix(np.array([[1.0, 0, 2], [0, 4, 0], [8, 0, 16]]))
    E, gone, bad = expected(X, 0.5, [1, 2, 0.5], [1, 1, 0.25], 0.5, prec)
    # (0,0): 1/2 * 1 * 1 = 1/2, not > 1/2.  (0,2): 1 * 1 * 1/4.  (1,1): 2 * 2 * 1 = 4.  (2,0): 4 * 1/2 * 1 = 2.  (2,2): 8 * 1/2 * 1/4 = 1.
    assert np.array_equal(E.toarray(), [[0, 0, 0], [0, 4, 0], [2, 0, 1]]) and E.nnz == 3 and (gone, bad) == (2, False)
    assert E.dtype == (np.float32 if prec else np.float64) and E.has_sorted_indices
    assert np.array_equal(E.indptr, [0, 0, 1, 3]) and np.array_equal(E.indices, [1, 0, 2])
    E, gone, bad = expected(X, 1.0, None, None, 0.0, prec)
    assert (E != X).nnz == 0 and (gone, bad) == (0, False)
    E, gone, bad = expected(X, 0.0, None, None, 0.0, prec)
    assert E.nnz == 0 and (gone, bad) == (5, False)


def test_the_order_of_the_multiplications_is_pinned():
    f = np.float32
    rng = np.random.default_rng(0)
    x, g, s = (rng.uniform(0.1, 9.0, 2000).astype(f) for _ in range(3))
    differ = np.flatnonzero((x * g) * s != x * (g * s))
    assert len(differ) > 0
    j = int(differ[0])
    X = sp.csr_matrix((np.array([x[j]]), ([1], [2])), shape=(3, 4))
    for su, si in (([0, s[j], 0], None), (None, [0, 0, s[j], 0])):
        E, gone, bad = expected(X, g[j], su, si, 0.0, True)
        assert E.data[0] == (x[j] * g[j]) * s[j] and E.data[0] != x[j] * (g[j] * s[j]) and (gone, bad) == (0, False)
    # the user scale before the item scale
    y, a, b = (rng.uniform(0.1, 9.0, 2000).astype(f) for _ in range(3))
    differ = np.flatnonzero((y * a) * b != (y * b) * a)
    assert len(differ) > 0
    j = int(differ[0])
    X = sp.csr_matrix((np.array([y[j]]), ([1], [2])), shape=(3, 4))
    E, _, _ = expected(X, 1.0, [0, a[j], 0], [0, 0, b[j], 0], 0.0, True)
    assert E.data[0] == (y[j] * a[j]) * b[j] and E.data[0] != (y[j] * b[j]) * a[j]


@PREC
def test_subnormal_underflow_and_overflow(prec):
    dt = np.float32 if prec else np.float64
    tiny, big = np.finfo(dt).tiny, np.finfo(dt).max
    X = sp.csr_matrix(np.array([[1.0, 0], [0, 3.0]]))
    g = float(tiny) / 16                                    # 1 * g and 3 * g are subnormal, and exact
    E, gone, bad = expected(X, g, None, None, 0.0, prec)
    assert (gone, bad) == (0, False) and np.array_equal(E.data, np.array([g, 3 * g], dt)) and (E.data > 0).all() and (E.data < tiny).all()
    E, gone, bad = expected(X, g, [dt(2) ** -60, 1], None, 0.0, prec)    # the first cell underflows to 0 and leaves
    assert (gone, bad) == (1, False) and E.nnz == 1 and E[1, 1] == dt(3 * g)
    X = sp.csr_matrix(np.array([[float(big) / 2, 0], [0, 3.0]]))
    assert expected(X, 1.0, [4, 1], None, 0.0, prec)[2] is True           # an overflow is reported
    assert expected(X, 1.0, [2, 1], None, 0.0, prec)[2] is False
    assert expected(X, 4.0, [0, 1], None, 0.0, prec)[2] is True           # inf * 0
