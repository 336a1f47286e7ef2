"""CPU-side checks of the batched top-N with per-item score weights (include/poismf_hip.h section 1o): the header's define equals the
api constant, the three symbols are declared with the agreed parameter names and exported by every flavour; the C entry point answers
2 / 0 without a device on the malformed cases, and never 2 for a row left short; the Python checks raise on the same cases before any
library call and shape the weights; the one scratch allocation stays inside the budget; and the reference the GPU tests compare
against gives hand-written answers."""
import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_gpu_topn_weighted import weighted_expect
from tests.test_topn_batch_cpu import BAD as BAD_BATCH, NITEMS, NUSERS, K, _NoDeviceSession, _define, _fake_fitted, _params
from tests.test_topn_deep_cpu import SHORT

NAMES = ("poismf_hip_topn_weighted", "poismf_hip_session_topn_weighted", "poismf_hip_topn_weighted_scratch_bytes")
ONES = [1.0] * NITEMS
MAX_ITEMS = api.TOPN_WEIGHTED_MAX_ITEMS   # (read at import: nothing in this file, the reference's check included, runs without the feature)

# section 1f's table; what is left after exclusion no longer matters
BAD = {c: v for c, v in BAD_BATCH.items() if c != "n-above-items-left"}
BAD_WEIGHTS = {
    "nan": ONES[:-1] + [float("nan")],
    "inf": [float("inf")] + ONES[1:],
    "negative": ONES[:7] + [-1e-30] + ONES[8:],
    "negative-inf": ONES[:7] + [float("-inf")] + ONES[8:],
    "null": None,
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_header_declares_the_prototypes_and_the_constants_agree():
    assert _params("poismf_hip_session_topn_weighted") == ("int", ["s", "users", "n_users", "n_top", "item_weight", "query_B", "exclude_seen",
                                                                   "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_weighted") == ("int", ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "item_weight",
                                                           "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_weighted_scratch_bytes") == ("size_t", ["n_users", "n_top", "dimB", "k"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_TOPN_WEIGHTED_MAX_ITEMS") == MAX_ITEMS == 2 ** 24


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_weighted(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def _c_call(flavour, users, n, excl, weight=ONES, n_users=None, dimB=NITEMS):
    """poismf_hip_topn_weighted itself through ctypes; index arrays in the flavour's sparse_ix, the weights in its real_t"""
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
    w = np.asarray(weight, dt) if weight is not None else None
    rc = lib.poismf_hip_topn_weighted(p(A), p(B), K, NUSERS, dimB, p(u), m, n, p(w) if w is not None else None,
                                      p(ip) if ip is not None else None, p(ii) if ii is not None else None, p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))   # (a C caller has no row count to get wrong)
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, n, excl = BAD[case]
    rc, out, sc = _c_call(flavour, users, n, excl)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD_WEIGHTS))
def test_c_entry_returns_2_on_malformed_weights(flavour, case):
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, weight=BAD_WEIGHTS[case])
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_too_many_items(flavour):
    """dimB = 2^24 + 1 is refused before the weights are read (the arrays here are far shorter)"""
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, dimB=2 ** 24 + 1)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u = np.zeros(1, np.uint64)
    w = np.ones(2, np.float32)
    out = np.zeros(1, np.uint64)
    p = api._ptr
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_weighted(p(A), p(A), k, 2, 2, p(u), 1, 1, p(w), None, None, p(out), None) == 2


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, _ = _c_call(flavour, [0], 5, None, n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_call(flavour, [0], 0, None, weight=None, n_users=0)   # (nothing else matters then)
    assert rc == 0


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(SHORT) + ["every-weight-zero"])
def test_c_entry_short_rows_and_zero_weights_are_not_an_argument_error(flavour, case):
    """past the checks the call needs a device: 0 where there is one, 1 where there is none, never 2"""
    if case in SHORT:
        users, n, excl = SHORT[case]
        if n > api.TOPN_BATCH_MAX_N_TOP:
            n = api.TOPN_BATCH_MAX_N_TOP   # (n-above-items: 128 items are not there either once 200 are excluded)
            excl = ([0, 200, 400], list(range(200)) * 2)
        rc, _, _ = _c_call(flavour, users, n, excl)
    else:
        rc, _, _ = _c_call(flavour, [0, 1], 5, None, weight=[0.0] * (NITEMS - 1) + [-0.0])
    assert rc in (0, 1)


# ---- Python ----
def test_the_calls_need_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_weighted([0, 1], item_weight=ONES)
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).similar_items([0, 1])


PY_BAD_WEIGHTS = {
    "missing": (None, "item_weight is required"),
    "too-short": (ONES[:-1], f"{NITEMS - 1} entries for {NITEMS} items"),
    "too-long": (ONES + [1.0], f"{NITEMS + 1} entries for {NITEMS} items"),
    "two-dimensional": ([ONES], "1-d array"),
    "nan": (BAD_WEIGHTS["nan"], "NaN"),
    "inf": (BAD_WEIGHTS["inf"], "infinite"),
    "negative": (BAD_WEIGHTS["negative"], "negative"),
    "negative-scalar": (-0.5, "negative"),
    "nan-scalar": (float("nan"), "NaN"),
    "text": (["a"] * NITEMS, "real numbers"),
    "flags": ([True] * NITEMS, "real numbers"),
}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_weighted(users, n, item_weight=ONES, exclude=excl)


@pytest.mark.parametrize("case", sorted(BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_weighted(users, n, item_weight=ONES, exclude=excl)


@pytest.mark.parametrize("case", sorted(PY_BAD_WEIGHTS))
def test_malformed_weights_raise_before_the_device(case):
    weight, message = PY_BAD_WEIGHTS[case]
    with pytest.raises(ValueError, match=message):
        _fake_fitted(True).topN_weighted([0, 1], 5, item_weight=weight)
    with pytest.raises(ValueError, match=message):
        _NoDeviceSession(True).topn_weighted([0, 1], 5, item_weight=weight)
    with pytest.raises(ValueError, match=message):
        api._topn_weighted_args([0, 1], 5, weight, None, NUSERS, NITEMS)


def test_a_weight_is_judged_after_the_conversion():
    """1e39 is a finite double and an infinite float; 1e-50 is a positive double and a zero float (accepted: 0 is a weight)"""
    big, tiny = ONES[:-1] + [1e39], ONES[:-1] + [1e-50]
    assert api._topn_weighted_args([0], 5, big, None, NUSERS, NITEMS, np.float64)[1][-1] == 1e39
    with pytest.raises(ValueError, match="infinite in the model's precision"):
        api._topn_weighted_args([0], 5, big, None, NUSERS, NITEMS, np.float32)
    with pytest.raises(ValueError, match="infinite in the model's precision"):
        _NoDeviceSession(True).topn_weighted([0], 5, item_weight=big)
    assert api._topn_weighted_args([0], 5, tiny, None, NUSERS, NITEMS, np.float32)[1][-1] == 0


def test_too_many_items_raise_before_the_device():
    s = _NoDeviceSession(True)
    s.dimB = MAX_ITEMS + 1
    with pytest.raises(ValueError, match="limit of 16777216"):
        s.topn_weighted([0, 1], 5, item_weight=1.0)
    with pytest.raises(ValueError, match="limit of 16777216"):
        s.similar_items([0, 1], 5)


def test_session_wrapper_exclude_seen_and_query_items():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_weighted([1, 5], 5, item_weight=ONES, exclude_seen=True)
    with pytest.raises(ValueError, match="exclude_seen has no meaning"):
        _NoDeviceSession(True).topn_weighted([1, 2], 5, item_weight=ONES, exclude_seen=True, query_items=True)
    with pytest.raises(ValueError, match="out of range"):
        _NoDeviceSession(True).topn_weighted([1, NUSERS], 5, item_weight=ONES)
    with pytest.raises(ValueError, match="out of range"):
        _NoDeviceSession(True).topn_weighted([1, NITEMS], 5, item_weight=ONES, query_items=True)
    with pytest.raises(AttributeError):                               # (an item index from dimA on passes the checks: the library is next)
        _NoDeviceSession(True).topn_weighted([1, NUSERS], 5, item_weight=ONES, query_items=True)


def test_similar_items_checks_before_the_device():
    for target in (_fake_fitted(True), _NoDeviceSession(True)):
        with pytest.raises(ValueError, match="out of range"):
            target.similar_items([0, NITEMS], 5, item_norm=ONES)
        with pytest.raises(ValueError, match="entries for"):
            target.similar_items([0, 1], 5, item_norm=ONES[:-1])
        with pytest.raises(ValueError, match="finite and non-negative"):
            target.similar_items([0, 1], 5, item_norm=ONES[:-1] + [-1.0])
        with pytest.raises(ValueError, match="above the batched limit"):
            target.similar_items([0, 1], 129, item_norm=ONES)
        # without item_norm the norms would be computed next, on a device: n and the items are judged before that
        with pytest.raises(ValueError, match="above the batched limit"):
            target.similar_items([0, 1], 129)
        with pytest.raises(ValueError, match="must be positive"):
            target.similar_items([0, 1], 0)
        with pytest.raises(ValueError, match="out of range"):
            target.similar_items([0, NITEMS], 5)
    inv = api._inv_norms([4.0, 0.0, 0.25], 3, np.float32)
    assert inv.dtype == np.float32 and inv.tolist() == [0.5, 0.0, 2.0]
    items, excl = api._similar_args([2, 0, 2], 5, True, 3)
    assert items.tolist() == [2, 0, 2] and excl[0].tolist() == [0, 1, 2, 3] and excl[1].tolist() == [2, 0, 2]
    assert api._similar_args([2, 0], 5, False, 3)[1] is None
    sc = np.array([[4.0, 2.0, -np.inf]], np.float32)
    assert api._similar_scores(sc, inv, np.array([1], np.uint64)).tolist() == [[0.0, 0.0, -np.inf]]   # (a zero query: 0, and the padding stays)


def test_python_checks_shape_the_arguments():
    """a scalar weight broadcasts over the items; an array is converted to the model's real_t; short rows are accepted"""
    u, w, indptr, indices = api._topn_weighted_args([0, 1], 5, 3, None, NUSERS, NITEMS, np.float32)
    assert u.dtype == np.uint64 and w.dtype == np.float32 and w.tolist() == [3.0] * NITEMS and indptr is None and indices is None
    w = api._topn_weighted_args([0, 1], 5, np.arange(NITEMS), None, NUSERS, NITEMS)[1]
    assert w.dtype == np.float64 and w.flags.c_contiguous and w.tolist() == list(range(NITEMS))
    w = api._topn_weighted_args([0, 1], 5, np.float32(0.1), None, NUSERS, NITEMS, np.float64)[1]
    assert w.dtype == np.float64 and w[0] == np.float64(np.float32(0.1))
    for case in sorted(SHORT):
        users, n, excl = SHORT[case]
        got = api._topn_weighted_args(users, min(n, 128), ONES, excl, NUSERS, NITEMS)
        assert (got[2] is None) == (excl is None)
    assert len(api._topn_weighted_args([], 5, 0, None, NUSERS, NITEMS)[0]) == 0


# ---- scratch ----
@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_scratch_stays_inside_the_budget(flavour):
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    assert budget == 256 << 20
    fn = api.load_library(flavour).poismf_hip_topn_weighted_scratch_bytes
    real = 4 if flavour is True else 8
    tops, items, batch = (1, 10, 128), (1, 40, 10 ** 5, 2 ** 24), (1, 64, 4096, 10 ** 6, 10 ** 7)
    size = {}
    for n in tops:
        for dimB in items:
            for m in batch:
                b = size[n, dimB, m] = int(fn(m, n, dimB, 50))
                assert 0 < b <= budget, (m, n, dimB, b)
                assert b >= real * dimB                                 # the weights
                for k in (1, 3, 512):
                    assert int(fn(m, n, dimB, k)) == b                  # no part depends on k
    for (n, dimB, m), b in size.items():
        later = [size[n, dimB, x] for x in batch]
        assert later == sorted(later)                                   # it never shrinks when the batch grows
    assert int(fn(64, 128, 1000, 50)) < (8 << 20)                       # a small call does not pay for a large one
    assert max(size.values()) > (budget >> 1)                           # (the bound is not vacuous)


# ---- the reference of tests/test_gpu_topn_weighted.py ----
def _answer(scores, weight, excl, n):
    ix, sc = weighted_expect(np.asarray([scores], np.float32), np.asarray(weight, np.float32), [excl], n)
    return ix[0].tolist(), sc[0].tolist()


def test_reference_on_hand_written_cases():
    NONE, ninf = api.TOPN_NONE, -np.inf
    #          item   0    1    2    3    4    5
    scores = [8.0, 6.0, 4.0, 3.0, 2.0, 1.0]
    # the weights reorder: 0.5, 1, 2, 1, 4, 0 -> 4, 6, 8, 3, 8, 0: items 2 and 4 tie at 8 and the smaller index leads
    w = [0.5, 1.0, 2.0, 1.0, 4.0, 0.0]
    assert _answer(scores, w, [], 4) == ([2, 4, 1, 0], [8.0, 8.0, 6.0, 4.0])
    assert _answer(scores, w, [2], 3) == ([4, 1, 0], [8.0, 6.0, 4.0])
    # a weight-0 item is listed, at score 0, once the row runs that deep; then the padding
    assert _answer(scores, w, [], 8) == ([2, 4, 1, 0, 3, 5, NONE, NONE], [8.0, 8.0, 6.0, 4.0, 3.0, 0.0, ninf, ninf])
    assert _answer(scores, [0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [3], 4) == ([2, 0, 1, 4], [4.0, 0.0, 0.0, 0.0])
    # every weight 1: the plain order; everything excluded: all padding
    assert _answer(scores, [1.0] * 6, [], 6) == (list(range(6)), scores)
    assert _answer(scores, w, list(range(6)), 2) == ([NONE, NONE], [ninf, ninf])
    # the product is made in the rows' precision: 3 x float32(0.1) rounded to float32, not the double product
    third = _answer([3.0], [0.1], [], 1)[1][0]
    assert third == float(np.float32(3.0) * np.float32(0.1)) and third != 3.0 * 0.1
