"""CPU-side checks of the deep batched top-N's boundary (include/poismf_hip.h section 1l): the header's two defines equal the api
constants, the three symbols are declared with the agreed parameter names and exported by every flavour; the one scratch allocation
of a call stays inside the stated budget and never shrinks when the batch grows; the C entry point answers 2 / 0 without a device
on section 1f's malformed cases (with the limit at 1025) but not for "n_top larger than what is left"; the Python checks raise on the
same cases before any library call; and topN_batch keeps its own limit."""
import os
import re

import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_topn_batch_cpu import BAD as BAD_BATCH, NITEMS, NUSERS, K, _NoDeviceSession, _fake_fitted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_topn_deep", "poismf_hip_session_topn_deep", "poismf_hip_topn_deep_scratch_bytes")

# section 1f's table with the limit moved; what is left after exclusion no longer matters
BAD = {**{c: v for c, v in BAD_BATCH.items() if c not in ("n-above-items-left", "n-above-limit")}, "n-above-limit": ([0, 1], 1025, None)}
SHORT = {
    "n-above-items-left": ([0, 1], 100, ([0, 0, 201], list(range(201)))),
    "n-above-items": ([0, 1], NITEMS + 1, None),
    "everything-excluded": ([0, 1], 5, ([0, NITEMS, NITEMS], list(range(NITEMS)))),
}


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


def test_header_declares_the_prototypes_and_the_constants_agree():
    # section 1f's argument order and types
    assert _params("poismf_hip_session_topn_deep") == _params("poismf_hip_session_topn_batch")
    assert _params("poismf_hip_session_topn_deep")[1] == ["s", "users", "n_users", "n_top", "exclude_seen", "excl_indptr", "excl_indices", "out_ix", "out_score"]
    assert _params("poismf_hip_topn_deep") == _params("poismf_hip_topn_batch")
    assert _params("poismf_hip_topn_deep_scratch_bytes") == ("size_t", ["n_users", "n_top", "dimB", "k"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_TOPN_DEEP_MAX_N_TOP") == api.TOPN_DEEP_MAX_N_TOP == 1024
    assert _define("POISMF_HIP_TOPN_DEEP_BUDGET_MB") == api.TOPN_DEEP_BUDGET_MB


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_deep(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def test_topn_deep_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_deep([0, 1])


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_stated_budget_and_never_shrinks(flavour):
    budget = _define("POISMF_HIP_TOPN_DEEP_BUDGET_MB") << 20
    fn = api.load_library(flavour).poismf_hip_topn_deep_scratch_bytes
    worst = 0
    for n in (1, 128, 129, 1024):
        for dimB in (1, 10 ** 5, 2 ** 31 - 1):
            before = 0
            for m in (1, 64, 4096, 10 ** 6, 10 ** 8):
                b = int(fn(m, n, dimB, 50))
                assert 0 < b <= budget, (m, n, dimB, b)
                assert b >= before, (m, n, dimB, b, before)   # (constant from the chunk size on)
                before = b
                worst = max(worst, b)
    assert int(fn(64, 128, 1000, 50)) < (8 << 20)         # a small call does not pay for a large one
    assert worst > (budget >> 1)                         # (the bound is not vacuous)
    # the header's own arithmetic: 512 workgroups' lists at n_top = 1024 fit beside a chunk's other parts
    entry = 8 if flavour else 12
    assert int(fn(10 ** 8, 1024, 10 ** 5, 50)) >= 64 * 512 * 2048 * entry


def _c_call(flavour, users, n, excl, n_users=None):
    """poismf_hip_topn_deep itself through ctypes; index arrays in the flavour's sparse_ix"""
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
    rc = lib.poismf_hip_topn_deep(p(A), p(B), K, NUSERS, NITEMS, p(u), m, n, p(ip) if ip is not None else None,
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
@pytest.mark.parametrize("case", sorted(SHORT))
def test_c_entry_short_rows_are_not_an_argument_error(flavour, case):
    """past the checks the call needs a device: 0 where there is one, 1 where there is none, never 2"""
    users, n, excl = SHORT[case]
    rc, _, _ = _c_call(flavour, users, n, excl)
    assert rc in (0, 1)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, _ = _c_call(flavour, [0], 5, None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_call(flavour, [0], 0, None, n_users=0)   # (not even n_top = 0 matters then)
    assert rc == 0


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u = np.zeros(1, np.uint64)
    out = np.zeros(1, np.uint64)
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_deep(api._ptr(A), api._ptr(A), k, 2, 2, api._ptr(u), 1, 1, None, None, api._ptr(out), None) == 2


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_deep(users, n, exclude=excl)


@pytest.mark.parametrize("case", sorted(BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_deep(users, n, exclude=excl)


def test_session_wrapper_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_deep([1, 5], 5, exclude_seen=True)


@pytest.mark.parametrize("case", sorted(SHORT))
def test_python_checks_accept_short_rows(case):
    users, n, excl = SHORT[case]
    u, indptr, indices = api._topn_deep_args(users, n, excl, NUSERS, NITEMS)
    assert u.dtype == np.uint64 and len(u) == 2
    assert (indptr is None) == (excl is None)
    users, indptr, indices = api._topn_deep_args([0, 1], 1024, None, NUSERS, NITEMS)
    assert indptr is None and indices is None


def test_the_shallow_call_keeps_its_limit():
    with pytest.raises(ValueError, match="batched limit of 128"):
        _fake_fitted(True).topN_batch([0, 1], 129)
    with pytest.raises(ValueError, match="batched limit of 128"):
        _NoDeviceSession(True).topn_batch([0, 1], 129)
    assert api.TOPN_BATCH_MAX_N_TOP == 128
