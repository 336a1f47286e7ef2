"""CPU-side checks of the likelihood's boundary (include/poismf_hip.h section 1e): the header declares eval_llk with the
reference's parameter list (ref: src/poismf.h:258-269) and poismf_hip_session_llk, every library flavour exports both, and
PoisMF.eval_llk rejects an unfitted model and out-of-range indices before anything reaches a device."""
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ref: src/poismf.h:258-269, as (type, name) with the restrict qualifiers dropped (C++ has none; run_poismf drops them too)
REF_EVAL_LLK = [("real_t *", "A"), ("real_t *", "B"), ("sparse_ix", "ixA[]"), ("sparse_ix", "ixB[]"), ("real_t *", "X"),
                ("size_t", "nnz"), ("int", "k"), ("bool", "full_llk"), ("bool", "include_missing"), ("size_t", "dimA"),
                ("size_t", "dimB"), ("int", "nthreads")]


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "poismf_hip.h")).read()
    m = re.search(r"^POISMF_HIP_API\s+([\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, f"{name} is not declared"
    params = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        t, n = re.match(r"(.*?)\s*(\w+(?:\[\])?)$", p).groups()
        params.append((t.strip(), n))
    return " ".join(m.group(1).split()), params


def test_header_declares_eval_llk_with_the_reference_prototype():
    ret, params = _prototype("eval_llk")
    assert ret == "long double"
    assert [(t.replace(" ", ""), n) for t, n in params] == [(t.replace(" ", ""), n) for t, n in REF_EVAL_LLK]


def test_header_declares_session_llk():
    ret, params = _prototype("poismf_hip_session_llk")
    assert ret == "int"
    assert [n for _, n in params] == ["s", "full_llk", "include_missing", "out"]
    assert "eval_llk" in api.EXPORTED_SYMBOLS and "poismf_hip_session_llk" in api.EXPORTED_SYMBOLS


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_llk(use_float):
    lib = api.load_library(use_float)
    for name in ("eval_llk", "poismf_hip_session_llk"):
        assert getattr(lib, name) is not None


def test_eval_llk_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).eval_llk(synth.readme_coo())


def _fake_fitted(use_float, nusers=4, nitems=6, k=3):
    """a model that looks fitted without any fit having run (no device is touched)"""
    m = api.PoisMF(k=k, use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((nusers, k), dt), np.ones((nitems, k), dt)
    m.nusers, m.nitems = nusers, nitems
    m.is_fitted = True
    return m


@pytest.mark.parametrize("use_float", [False, True])
@pytest.mark.parametrize("row,col", [([0, 4], [1, 2]), ([0, 1], [5, 6]), ([-1, 0], [0, 0]), ([0, 0], [0, -3])],
                         ids=["user", "item", "negative-user", "negative-item"])
def test_out_of_range_indices_raise_before_the_device(use_float, row, col):
    m = _fake_fitted(use_float)
    t = synth.Triplets(np.array(row, np.int64), np.array(col, np.int64), np.array([1.0, 2.0]), (10, 10))
    with pytest.raises(IndexError):
        m.eval_llk(t)


def test_out_of_range_scipy_matrix_raises():
    import scipy.sparse as sp
    m = _fake_fitted(True)
    X = sp.csr_matrix((np.array([1.0]), (np.array([0]), np.array([6]))), shape=(4, 7))
    with pytest.raises(IndexError):
        m.eval_llk(X, full_llk=True, include_missing=True)
