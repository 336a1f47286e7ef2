"""CPU-side checks of the batched top-N with per-(user, item) score factors (include/poismf_hip.h section 1r): the header's defines
equal the api constants, the four symbols are declared with the agreed parameter names and exported by every flavour; the C entry
point answers 2 / 0 without a device on the malformed cases, and never 2 for a row left short or a factor of 0; the Python checks raise
on the same cases before any library call and shape the adjust list; the one scratch allocation stays inside the budget; and the
reference the GPU tests compare against gives hand-written answers."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build
from tests.test_gpu_topn_adjusted import adj_triple, adjusted_expect
from tests.test_topn_batch_cpu import BAD as BAD_BATCH, NITEMS, NUSERS, K, _NoDeviceSession, _define, _fake_fitted, _params
from tests.test_topn_deep_cpu import SHORT

NAMES = ("poismf_hip_topn_adjusted", "poismf_hip_session_topn_adjusted", "poismf_hip_topn_adjusted_scratch_bytes", "poismf_hip_topn_adjusted_slices")
MAX_ITEMS, MAX_ROW = api.TOPN_ADJUSTED_MAX_ITEMS, api.TOPN_ADJUSTED_MAX_ROW   # (read at import: nothing in this file runs without the feature)
NOTHING = ([0, 0, 0], [], [])       # two users, no cell listed
GOOD = ([0, 2, 3], [1, 7, 4], [0.5, 2.0, 0.0])

# section 1f's table; what is left after exclusion no longer matters
BAD = {c: v for c, v in BAD_BATCH.items() if c != "n-above-items-left"}
# (indptr, indices, factors) for users [0, 1]: every one malformed
BAD_ADJUST = {
    "pointers-decrease": ([0, 2, 1], [1, 2], [1.0, 1.0]),
    "pointers-start-below-zero": ([-1, 0, 1], [1, 2], [1.0, 1.0]),
    "item-out-of-range": ([0, 1, 2], [3, NITEMS], [1.0, 1.0]),
    "negative-item": ([0, 1, 2], [-2, 4], [1.0, 1.0]),
    "descending-row": ([0, 2, 4], [1, 2, 9, 7], [1.0] * 4),
    "repeated-item": ([0, 2, 4], [1, 2, 7, 7], [1.0] * 4),
    "nan": ([0, 2, 3], [1, 7, 4], [1.0, float("nan"), 1.0]),
    "inf": ([0, 2, 3], [1, 7, 4], [float("inf"), 1.0, 1.0]),
    "negative": ([0, 2, 3], [1, 7, 4], [1.0, 1.0, -1e-30]),
    "negative-inf": ([0, 2, 3], [1, 7, 4], [1.0, float("-inf"), 1.0]),
    "no-factors": ([0, 2, 3], [1, 7, 4], None),
    "no-indices": ([0, 2, 3], None, [1.0, 1.0, 1.0]),
    "null": (None, None, None),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_header_declares_the_prototypes_and_the_constants_agree():
    assert _params("poismf_hip_session_topn_adjusted") == ("int", ["s", "users", "n_users", "n_top", "adj_indptr", "adj_indices", "adj_factor",
                                                                   "exclude_seen", "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_adjusted") == ("int", ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "adj_indptr", "adj_indices",
                                                           "adj_factor", "excl_indptr", "excl_indices", "out_ix", "out_score"])
    assert _params("poismf_hip_topn_adjusted_scratch_bytes") == ("size_t", ["n_users", "n_cells", "n_top", "dimB", "k"])
    assert _params("poismf_hip_topn_adjusted_slices") == ("size_t", ["len", "n_top", "bound"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_TOPN_ADJUSTED_MAX_ITEMS") == MAX_ITEMS == 2 ** 24
    assert _define("POISMF_HIP_TOPN_ADJUSTED_MAX_ROW") == MAX_ROW == 2 ** 22


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_adjusted(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def _c_call(flavour, users, n, excl, adjust=NOTHING, n_users=None, dimB=NITEMS):
    """poismf_hip_topn_adjusted itself through ctypes; index arrays in the flavour's sparse_ix, the factors in its real_t"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        if a is None:
            return None
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    out = np.full((max(m, 1), max(n, 1)), 12345, it)
    sc = np.full((max(m, 1), max(n, 1)), -7.0, dt)
    p = lambda a: api._ptr(a) if a is not None and len(a) else None
    ip, ii = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    ap, ai = ix(adjust[0]), ix(adjust[1])
    af = np.asarray(adjust[2], dt) if adjust[2] is not None else None
    rc = lib.poismf_hip_topn_adjusted(p(A), p(B), K, NUSERS, dimB, p(u), m, n, p(ap), p(ai), p(af), p(ip), p(ii), p(out), p(sc))
    return rc, out, sc


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))   # (a C caller has no row count to get wrong)
@pytest.mark.parametrize("adjust", [NOTHING, GOOD], ids=["nothing-listed", "cells-listed"])
def test_c_entry_returns_2_and_writes_nothing(flavour, case, adjust):
    users, n, excl = BAD[case]
    rc, out, sc = _c_call(flavour, users, n, excl, adjust=adjust)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD_ADJUST))
def test_c_entry_returns_2_on_a_malformed_adjust_list(flavour, case):
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, adjust=BAD_ADJUST[case])
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_row_over_the_limit_and_too_many_items(flavour):
    """a row of 2^22 + 1 cells is refused by its row pointers, before a cell is read (the arrays here are far shorter); so is
    dimB = 2^24 + 1"""
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, adjust=([0, MAX_ROW + 1, MAX_ROW + 1], [0, 1], [1.0, 1.0]), dimB=2 ** 23)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)
    rc, out, sc = _c_call(flavour, [0, 1], 5, None, dimB=2 ** 24 + 1)
    assert rc == 2
    assert np.all(out == 12345) and np.all(sc == -7.0)


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u = np.zeros(1, np.uint64)
    ap = np.zeros(2, np.uint64)
    out = np.zeros(1, np.uint64)
    p = api._ptr
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_adjusted(p(A), p(A), k, 2, 2, p(u), 1, 1, p(ap), None, None, None, None, p(out), None) == 2


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, out, _ = _c_call(flavour, [0], 5, None, adjust=([0, 0], [], []), n_users=0)
    assert rc == 0 and np.all(out == 12345)
    rc, _, _ = _c_call(flavour, [0], 0, None, adjust=(None, None, None), n_users=0)   # (nothing else matters then)
    assert rc == 0


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(SHORT) + ["every-factor-zero", "listed-and-excluded"])
def test_c_entry_short_rows_and_zero_factors_are_not_an_argument_error(flavour, case):
    """past the checks the call needs a device: 0 where there is one, 1 where there is none, never 2"""
    if case in SHORT:
        users, n, excl = SHORT[case]
        if n > api.TOPN_BATCH_MAX_N_TOP:
            n = api.TOPN_BATCH_MAX_N_TOP   # (n-above-items: 128 items are not there either once 200 are excluded)
            excl = ([0, 200, 400], list(range(200)) * 2)
        rc, _, _ = _c_call(flavour, users, n, excl, adjust=GOOD)
    elif case == "every-factor-zero":
        rc, _, _ = _c_call(flavour, [0, 1], 5, None, adjust=([0, 2, 3], [1, 7, 4], [0.0, -0.0, 0.0]))
    else:
        rc, _, _ = _c_call(flavour, [0, 1], 5, ([0, 2, 3], [1, 7, 4]), adjust=GOOD)
    assert rc in (0, 1)


# ---- Python ----
def test_the_call_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_adjusted([0, 1], adjust=GOOD)


PY_BAD_ADJUST = {
    **{c: (v, None) for c, v in BAD_ADJUST.items() if c not in ("null", "no-factors", "no-indices", "pointers-start-below-zero")},
    "nan": (BAD_ADJUST["nan"], "NaN"),
    "inf": (BAD_ADJUST["inf"], "infinite"),
    "negative": (BAD_ADJUST["negative"], "negative"),
    "pointers-leave-the-list": (([0, 2, 4], [1, 7, 4], [1.0] * 3), "stay inside"),
    "fewer-factors-than-indices": (([0, 2, 3], [1, 7, 4], [1.0, 1.0]), "fewer factors"),
    "a-pair": (([0, 2, 3], [1, 7, 4]), "triple"),
    "wrong-rows": (([0, 1, 2, 3], [1, 2, 3], [1.0] * 3), "rows for 2 users"),
    "matrix-wrong-rows": (sp.csr_matrix((3, NITEMS)), "3 rows for 2 users"),
    "matrix-too-wide": (sp.csr_matrix((2, NITEMS + 1)), "more columns"),
    "a-dense-array": (np.ones((2, NITEMS)), "SciPy sparse matrix"),
    "text": (([0, 2, 3], [1, 7, 4], ["a", "b", "c"]), "real numbers"),
    "flags": (([0, 2, 3], [1, 7, 4], [True, False, True]), "real numbers"),
    "two-dimensional-factors": (([0, 2, 3], [1, 7, 4], [[1.0, 1.0, 1.0]]), "1-d array"),
    "matrix-negative": (sp.csr_matrix(([1.0, -2.0], ([0, 1], [3, 4])), shape=(2, NITEMS)), "negative"),
}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_adjusted(users, n, adjust=NOTHING, exclude=excl)


@pytest.mark.parametrize("case", sorted(BAD))
def test_session_wrapper_raises_before_the_device(case):
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).topn_adjusted(users, n, adjust=NOTHING, exclude=excl)


@pytest.mark.parametrize("case", sorted(PY_BAD_ADJUST))
def test_a_malformed_adjust_list_raises_before_the_device(case):
    adjust, message = PY_BAD_ADJUST[case]
    with pytest.raises(ValueError, match=message):
        _fake_fitted(True).topN_adjusted([0, 1], 5, adjust=adjust)
    with pytest.raises(ValueError, match=message):
        _NoDeviceSession(True).topn_adjusted([0, 1], 5, adjust=adjust)
    with pytest.raises(ValueError, match=message):
        api._topn_adjusted_args([0, 1], 5, adjust, None, NUSERS, NITEMS)


def test_a_factor_is_judged_after_the_conversion():
    """1e39 is a finite double and an infinite float; 1e-50 is a positive double and a zero float (accepted: 0 is a factor)"""
    big, tiny = ([0, 1, 2], [3, 4], [1.0, 1e39]), ([0, 1, 2], [3, 4], [1.0, 1e-50])
    assert api._topn_adjusted_args([0, 1], 5, big, None, NUSERS, NITEMS, np.float64)[3][-1] == 1e39
    with pytest.raises(ValueError, match="infinite in the model's precision"):
        api._topn_adjusted_args([0, 1], 5, big, None, NUSERS, NITEMS, np.float32)
    with pytest.raises(ValueError, match="infinite in the model's precision"):
        _NoDeviceSession(True).topn_adjusted([0, 1], 5, adjust=big)
    with pytest.raises(ValueError, match="infinite in the model's precision"):
        _fake_fitted(True).topN_adjusted([0, 1], 5, adjust=sp.csr_matrix(([1e39], ([1], [4])), shape=(2, NITEMS)))
    assert api._topn_adjusted_args([0, 1], 5, tiny, None, NUSERS, NITEMS, np.float32)[3][-1] == 0


def test_limits_raise_before_the_device():
    s = _NoDeviceSession(True)
    with pytest.raises(ValueError, match="outside"):
        s.topn_adjusted([1, 5], 5, adjust=NOTHING, exclude_seen=True)
    s.dimB = MAX_ITEMS + 1
    with pytest.raises(ValueError, match="limit of 16777216"):
        s.topn_adjusted([0, 1], 5, adjust=NOTHING)
    s.dimB = 2 ** 23
    with pytest.raises(ValueError, match=f"longer than {MAX_ROW}"):
        s.topn_adjusted([0, 1], 5, adjust=([0, MAX_ROW + 1, MAX_ROW + 1], np.arange(MAX_ROW + 1), np.ones(MAX_ROW + 1, np.float32)))
    assert len(api._topn_adjusted_args([0, 1], 5, ([0, MAX_ROW, MAX_ROW], np.arange(MAX_ROW), np.ones(MAX_ROW, np.float32)), None, NUSERS, 2 ** 23)[2]) == MAX_ROW


def test_python_checks_shape_the_arguments():
    """None lists nothing; a triple may start anywhere; a SciPy matrix keeps its stored zeros, is sorted and converted to the model's
    real_t; short rows are accepted"""
    u, ap, ai, f, indptr, indices = api._topn_adjusted_args([0, 1], 5, None, None, NUSERS, NITEMS, np.float32)
    assert u.dtype == np.uint64 and ap.tolist() == [0, 0, 0] and ap.dtype == np.uint64 and len(ai) == 0 and len(f) == 0 and f.dtype == np.float32
    assert indptr is None and indices is None
    _, ap, ai, f, _, _ = api._topn_adjusted_args([0, 1], 5, ([1, 3, 4], [99, 1, 7, 4, 98], [9, 0.5, 2, 0, 9]), None, NUSERS, NITEMS)
    assert ap.tolist() == [0, 2, 3] and ai.tolist() == [1, 7, 4] and f.tolist() == [0.5, 2.0, 0.0] and f.dtype == np.float64
    assert ai.dtype == np.uint64 and f.flags.c_contiguous
    # stored zeros are kept, unsorted indices sorted with their factors, and the caller's matrix is left as it was
    mat = sp.csr_matrix((np.array([3.0, 0.0, 0.25]), np.array([7, 1, 4]), np.array([0, 2, 3])), shape=(2, NITEMS))
    _, ap, ai, f, _, _ = api._topn_adjusted_args([0, 1], 5, mat, None, NUSERS, NITEMS, np.float32)
    assert ap.tolist() == [0, 2, 3] and ai.tolist() == [1, 7, 4] and f.tolist() == [0.0, 3.0, 0.25] and f.dtype == np.float32
    assert mat.indices.tolist() == [7, 1, 4] and mat.data.tolist() == [3.0, 0.0, 0.25]
    X = sp.random(NUSERS, NITEMS, 0.05, format="csr", random_state=1)
    adj = X[[4, 0, 4]].copy()
    adj.data[:] = 0.5
    _, ap, ai, f, _, _ = api._topn_adjusted_args([4, 0, 4], 5, adj, None, NUSERS, NITEMS)
    assert ap.tolist() == adj.indptr.tolist() and ai.tolist() == adj.indices.tolist() and set(f.tolist()) == {0.5}
    _, _, _, f, _, _ = api._topn_adjusted_args([0, 1], 5, ([0, 1, 2], [3, 4], np.array([1, 2])), None, NUSERS, NITEMS, np.float32)
    assert f.dtype == np.float32 and f.tolist() == [1.0, 2.0]
    for case in sorted(SHORT):
        users, n, excl = SHORT[case]
        got = api._topn_adjusted_args(users, min(n, 128), GOOD, excl, NUSERS, NITEMS)
        assert (got[4] is None) == (excl is None)
    assert len(api._topn_adjusted_args([], 5, None, None, NUSERS, NITEMS)[0]) == 0


# ---- scratch ----
@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_scratch_stays_inside_the_budget(flavour):
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    assert budget == 256 << 20
    fn = api.load_library(flavour).poismf_hip_topn_adjusted_scratch_bytes
    real = 4 if flavour is True else 8
    tops, items, batch = (1, 10, 128), (1, 40, 10 ** 5, 2 ** 24), (1, 64, 4096, 10 ** 6, 10 ** 7)
    cells = (0, 1, 100, 10 ** 5, MAX_ROW, 10 ** 8, 10 ** 10)
    size = {}
    for n in tops:
        for dimB in items:
            for m in batch:
                for c in cells:
                    b = size[n, dimB, m, c] = int(fn(m, c, n, dimB, 50))
                    assert 0 < b <= budget, (m, c, n, dimB, b)
                    assert b >= min(c, MAX_ROW) * (4 + real)            # the adjust area: index and factor
                    assert b >= m * 4 if m <= 4096 else True
                for k in (1, 3, 512):
                    assert int(fn(m, 100, n, dimB, k)) == size[n, dimB, m, 100]   # no part depends on k
    assert int(fn(64, 6400, 128, 1000, 50)) < (8 << 20)                 # a small call does not pay for a large one
    assert max(size.values()) > (budget >> 1)                           # (the bound is not vacuous)


# ---- the plan of the sparse stage ----
@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_the_chunk_cut_charges_a_row_no_less_than_any_shorter_row_takes(flavour):
    """A row's work items are not monotone in its length (the cells per work item are rounded up to 64), and a row loses cells to the
    exclusion list after the chunk was cut.  What the cut charges -- slices(len, n, 1) -- never decreases with len, is no less than the
    work items of ANY row of at most len cells, and allows a user no more lists than the merge ranks: 2048 / n entries, half of them
    the dense stage's.  Every length up to 700 000 at n = 10, where the windows lie, in the double flavour (the function does not
    depend on real_t or sparse_ix); strides and the neighbourhood of every multiple of 64 x the most work items elsewhere"""
    fn = api.load_library(flavour).poismf_hip_topn_adjusted_slices
    assert (int(fn(104449, 10, 0)), int(fn(104448, 10, 0))) == (97, 102)     # the count itself does fall when a row grows
    assert int(fn(104449, 10, 1)) >= 102
    assert int(fn(0, 10, 0)) == int(fn(0, 10, 1)) == 0 and int(fn(1, 10, 0)) == int(fn(1, 10, 1)) == 1
    for n in (1, 10, 100, 128):
        most = 2048 // n - (2048 // n) // 2
        if n == 10 and flavour is False:
            lens = np.arange(0, 700001)
        else:
            near = (np.arange(1, 40)[:, None] * (most * 64) + np.arange(-3, 4)[None, :]).reshape(-1)
            lens = np.unique(np.r_[np.arange(0, MAX_ROW + 1, 4093), near[near <= MAX_ROW], 1024 * most + np.arange(-2, 3), MAX_ROW])
        took = np.array([int(fn(int(c), n, 0)) for c in lens])
        charged = np.array([int(fn(int(c), n, 1)) for c in lens])
        assert took.max() <= most and charged.max() <= most
        assert np.all(np.diff(charged) >= 0)                                   # monotone
        assert np.all(charged >= np.maximum.accumulate(took))                  # no less than any shorter row of the scan takes
        short = lens <= 1024 * most
        assert np.all(took[lens > 0] >= 1) and np.array_equal(took[short], -(-lens[short] // 1024))   # slices of 1024 cells while the merge allows
        if n == 10 and flavour is False:
            assert np.any(np.diff(took) < 0)                                   # (the scan does contain the windows)


# ---- the reference of tests/test_gpu_topn_adjusted.py ----
def _answer(scores, cells, factors, excl, n):
    ix, sc = adjusted_expect(np.asarray([scores], np.float32), [(cells, np.asarray(factors, np.float32))], [excl], n)
    return ix[0].tolist(), sc[0].tolist()


def test_reference_on_hand_written_cases():
    NONE, ninf = api.TOPN_NONE, -np.inf
    #          item   0    1    2    3    4    5
    scores = [8.0, 6.0, 4.0, 3.0, 2.0, 1.0]
    # cells 0, 2, 4, 5 at 0.5, 2, 4, 0 -> 4, 6, 8, 3, 8, 0: items 2 and 4 tie at 8 and the smaller index leads; the unlisted item 1
    # (6) and the listed item 0 (4) follow
    cells, f = [0, 2, 4, 5], [0.5, 2.0, 4.0, 0.0]
    assert _answer(scores, cells, f, [], 4) == ([2, 4, 1, 0], [8.0, 8.0, 6.0, 4.0])
    assert _answer(scores, cells, f, [2], 3) == ([4, 1, 0], [8.0, 6.0, 4.0])          # a cell listed and excluded is excluded
    # a factor-0 cell is listed, at score 0, once the row runs that deep; then the padding
    assert _answer(scores, cells, f, [], 8) == ([2, 4, 1, 0, 3, 5, NONE, NONE], [8.0, 8.0, 6.0, 4.0, 3.0, 0.0, ninf, ninf])
    # a listed item ties with an unlisted one: 1 x 0.5 = 3 and item 3 = 3; the smaller index leads
    assert _answer(scores, [1], [0.5], [], 6) == ([0, 2, 1, 3, 4, 5], [8.0, 4.0, 3.0, 3.0, 2.0, 1.0])
    # nothing listed, or factors of 1: the plain order; everything excluded: all padding
    assert _answer(scores, [], [], [], 6) == (list(range(6)), scores)
    assert _answer(scores, [0, 3], [1.0, 1.0], [], 6) == (list(range(6)), scores)
    assert _answer(scores, cells, f, list(range(6)), 2) == ([NONE, NONE], [ninf, ninf])
    # the product is made in the rows' precision: 3 x float32(0.1) rounded to float32, not the double product
    third = _answer([3.0], [0], [0.1], [], 1)[1][0]
    assert third == float(np.float32(3.0) * np.float32(0.1)) and third != 3.0 * 0.1
    # the triple the calls take
    ap, ai, af = adj_triple([([1, 7], [0.5, 2.0]), ([], []), ([4], [0.0])], np.float32)
    assert ap.tolist() == [0, 2, 2, 3] and ai.tolist() == [1, 7, 4] and af.tolist() == [0.5, 2.0, 0.0] and af.dtype == np.float32
