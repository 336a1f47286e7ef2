"""CPU-side checks of the list-wise evaluation (include/poismf_hip.h section 1q): the header's defines equal the api constants, the
three symbols are declared and exported; the Python checks raise on malformed input before any library is loaded; metrics.py's list
metrics against hand-written answers; and the numpy reference the GPU tests compare with (lists_expect) against hand-written answers,
the clamp, the NaN rule and a tie at half in the rounding among them."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, metrics
from tests.test_topn_batch_cpu import HEADER, NITEMS, NUSERS, K, _NoDeviceSession, _fake_fitted, _params

NAMES = ("poismf_hip_list_eval", "poismf_hip_session_list_eval", "poismf_hip_list_eval_scratch_bytes")
NONE = api.TOPN_NONE


# ---- the reference of the GPU tests ----
def lists_expect(lists, chains, inv, test, dimB):
    """Section 1q in numpy.  lists: uint64 [m x n], rows padded with TOPN_NONE.  chains(P): the [c x c] fused chains among the rows of B
    of the items P, in the model's dtype -- chains(P)[q, p] = chain(B[P[q]], B[P[p]]).  inv: [dimB] inverse norms in the same dtype, or
    None.  test: (indptr, indices) of the held-out rows, or None.  The two multiplications are single numpy operations in the model's
    dtype, in the header's order; the quantisation is np.rint on a double, then an integer sum.  Returns (pos uint32 or None, cos_sum
    int64 or None, length uint32, exposure uint32)."""
    lists = np.asarray(lists, np.uint64)
    m = lists.shape[0]
    rows = [r[r != NONE].astype(np.int64) for r in lists]
    length = np.array([len(r) for r in rows], np.uint32).reshape(m)
    expo = np.bincount(np.concatenate(rows + [np.empty(0, np.int64)]), minlength=dimB).astype(np.uint32)
    cos = None
    if inv is not None:
        inv = np.asarray(inv)
        cos = np.zeros(m, np.int64)
        for u, P in enumerate(rows):
            if len(P) < 2:
                continue
            G = chains(P)
            assert G.dtype == inv.dtype and G.shape == (len(P), len(P))
            with np.errstate(invalid="ignore", over="ignore"):
                cs = np.multiply(np.multiply(G, inv[P][:, None]), inv[P][None, :])   # [q, p]: (chain x inv[jq]) x inv[jp]
            assert cs.dtype == inv.dtype
            t = cs.astype(np.float64)
            Q = np.rint(np.clip(np.where(np.isnan(t), 0, t), -2, 2) * 2.0 ** 40).astype(np.int64)
            cos[u] = Q[np.tril_indices(len(P), -1)].sum()                             # the pairs p < q
    pos = None
    if test is not None:
        tp, ti = np.asarray(test[0], np.int64), np.asarray(test[1], np.int64)
        pos = np.full(len(ti), api.LIST_ABSENT, np.uint32)
        for u in range(m):
            where = {int(j): p for p, j in enumerate(rows[u])}
            for cell in range(tp[u], tp[u + 1]):
                if int(ti[cell]) in where:
                    pos[cell] = where[int(ti[cell])]
    return pos, cos, length, expo


def _chains_of(table):
    table = np.asarray(table)
    return lambda P: table[np.ix_(P, P)]


def test_lists_expect_on_a_hand_written_case():
    # three items with unit norms: cosines 0.5, 0.25, 0.125
    G = np.array([[1, .5, .25], [.5, 1, .125], [.25, .125, 1]])
    lists = np.array([[2, 0, 1], [1, NONE, NONE], [NONE, NONE, NONE], [0, 2, NONE]], np.uint64)
    test = ([0, 3, 4, 5, 5], [0, 1, 3, 1, 2])
    pos, cos, length, expo = lists_expect(lists, _chains_of(G), np.ones(4), test, 4)
    A = api.LIST_ABSENT
    assert pos.tolist() == [1, 2, A, 0, A] and pos.dtype == np.uint32
    assert cos.tolist() == [int((.5 + .25 + .125) * 2 ** 40), 0, 0, 2 ** 38] and cos.dtype == np.int64
    assert length.tolist() == [3, 1, 0, 2] and expo.tolist() == [2, 2, 2, 0]
    none = lists_expect(lists, _chains_of(G), None, None, 4)
    assert none[0] is None and none[1] is None and none[2].tolist() == [3, 1, 0, 2]


def test_lists_expect_order_of_the_two_multiplications():
    """(chain x inv[later]) x inv[earlier]: in float32 the other order rounds differently here"""
    g, a, b = np.float32(0.6369616985321045), np.float32(0.2697867155075073), np.float32(0.04097352549433708)
    assert (g * a) * b != (g * b) * a
    G = np.array([[1, g], [g, 1]], np.float32)
    inv = np.array([b, a], np.float32)            # item 0 is listed first (the earlier), item 1 later
    _, cos, _, _ = lists_expect(np.array([[0, 1]], np.uint64), _chains_of(G), inv, None, 2)
    assert cos[0] == int(np.rint(float((g * a) * b) * 2.0 ** 40))
    _, cos, _, _ = lists_expect(np.array([[1, 0]], np.uint64), _chains_of(G), inv, None, 2)
    assert cos[0] == int(np.rint(float((g * b) * a) * 2.0 ** 40))


def test_lists_expect_clamp_nan_and_ties_at_half():
    h = 2.0 ** -40
    G = np.zeros((8, 8))
    G[1, 0] = G[0, 1] = 3.0            # above the clamp: counts as 2
    G[3, 2] = G[2, 3] = -7.0           # below: -2
    G[5, 4] = G[4, 5] = np.inf         # times an inverse norm of 0: NaN, counts as 0
    G[7, 6] = G[6, 7] = 2.5 * h        # a tie at half: to the even neighbour, 2
    inv = np.ones(8)
    inv[4] = 0
    pairs = np.array([[0, 1], [2, 3], [4, 5], [6, 7]], np.uint64)
    _, cos, _, _ = lists_expect(pairs, _chains_of(G), inv, None, 8)
    assert cos.tolist() == [2 ** 41, -2 ** 41, 0, 2]
    G[7, 6] = G[6, 7] = 3.5 * h        # the other way: 4
    G[1, 0] = G[0, 1] = -0.5 * h       # -0.5 goes to 0, and 1.5 (below) to 2
    G[3, 2] = G[2, 3] = 1.5 * h
    _, cos, _, _ = lists_expect(pairs, _chains_of(G), inv, None, 8)
    assert cos.tolist() == [0, 2, 0, 4]


# ---- the header ----
def _define_any(name):
    m = re.search(r"^#define\s+" + name + r"\s+(0[xX][0-9a-fA-F]+|\d+)[uU]?\b", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1), 0)


def test_header_declares_the_prototypes_and_the_constants_agree():
    tail = ["item_inv_norm", "test_indptr", "test_indices", "budget_bytes", "out_pos", "out_cos", "out_len", "exposure"]
    assert _params("poismf_hip_list_eval") == ("int", ["B", "k", "dimB", "lists", "n_users", "n_list"] + tail)
    assert _params("poismf_hip_session_list_eval") == ("int", ["s", "lists", "n_users", "n_list"] + tail)
    assert _params("poismf_hip_list_eval_scratch_bytes") == ("size_t", ["n_users", "n_list", "n_cells", "dimB", "budget_bytes"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define_any("POISMF_HIP_LIST_ABSENT") == api.LIST_ABSENT == metrics.LIST_ABSENT == 0xFFFFFFFE
    assert _define_any("POISMF_HIP_LIST_COS_SHIFT") == api.LIST_COS_SHIFT == metrics.LIST_COS_SHIFT == 40
    assert _define_any("POISMF_HIP_LIST_EVAL_BUDGET_MB") == api.LIST_EVAL_BUDGET_MB == 256
    assert _define_any("POISMF_HIP_LIST_EVAL_MAX_ITEMS") == api.LIST_EVAL_MAX_ITEMS == 2 ** 24
    assert api.LIST_ABSENT != api.RANK_EXCLUDED


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_list_eval(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def test_the_host_arithmetic_of_the_scratch_is_the_library_s():
    lib = api.load_library(True)
    for m, n, cells, dimB, budget in ((150, 10, 900, 700, 0), (150, 10, 900, 700, 14000), (150, 128, 0, 700, 30000), (1, 1, 0, 1, 300),
                                      (10 ** 6, 10, 10 ** 7, 10 ** 5, 0), (10 ** 6, 128, 10 ** 9, 2 ** 24, 0), (3, 10, 70000, 700, 10 ** 6),
                                      (150, 10, 900, 700, 8000), (5, 5, 5, 2 ** 24 + 5, 1 << 40)):
        got = lib.poismf_hip_list_eval_scratch_bytes(m, n, cells, dimB, budget)
        assert got == api._list_eval_scratch(m, n, cells, dimB, budget, 4)[0], (m, n, cells, dimB, budget)
        assert got <= (budget if 0 < budget < 256 << 20 else 256 << 20)
    assert lib.poismf_hip_list_eval_scratch_bytes(150, 10, 900, 700, 8000) == 0       # below the norms, the counts and the 900 cells
    assert 0 < lib.poismf_hip_list_eval_scratch_bytes(150, 10, 900, 700, 14000) <= 14000
    assert api.load_library(False).poismf_hip_list_eval_scratch_bytes(10 ** 6, 128, 10 ** 9, 2 ** 24, 0) <= 256 << 20


@pytest.mark.parametrize("flavour", [False, True, "r"])
def test_c_check_finds_a_repeat_in_full_rows_and_accepts_distinct_ones(flavour):
    """the C check makes no device call: 2 for a repeated entry anywhere in rows of 128, and never 2 for distinct rows (past the checks
    the call needs a device: 0 where there is one, 1 where there is none)"""
    lib = api.load_library(flavour)
    p = api._ptr
    ix = np.int32 if flavour == "r" else np.uint64
    dimB, k, m, n = 40000, 3, 40, 128
    B = np.ones((dimB, k), np.float32 if flavour is True else np.float64)
    rng = np.random.default_rng(3)
    good = np.stack([rng.permutation(dimB)[:n] for _ in range(m)])
    good[1] = np.arange(n) * 256                                   # (multiples of 256, and a row equal to its neighbour)
    good[2] = good[1]

    def call(lists):
        lists = np.ascontiguousarray(lists, dtype=ix)
        length, expo = np.full(m, 12345, np.uint32), np.full(dimB, 12345, np.uint32)
        return lib.poismf_hip_list_eval(p(B), k, dimB, p(lists), m, n, None, None, None, 0, None, None, p(length), p(expo)), length, expo

    assert call(good)[0] in (0, 1)
    for row, a, b in ((0, 0, 127), (39, 126, 127), (17, 5, 6), (2, 64, 3)):
        bad = good.copy()
        bad[row, b] = bad[row, a]
        rc, length, expo = call(bad)
        assert rc == 2 and np.all(length == 12345) and np.all(expo == 12345), (row, a, b)


# ---- the Python checks, before any library is loaded ----
GOOD = [[3, 1, 2], [5, 4, NONE]]
ONES = [1.0] * NITEMS
BAD_LISTS = {
    "repeated-entry": [[3, 1, 3], [5, 4, NONE]],
    "entry-after-padding": [[3, 1, 2], [5, NONE, 4]],
    "index-out-of-range": [[3, 1, NITEMS], [5, 4, NONE]],
    "negative-index": np.array([[3, 1, -1], [5, 4, 0]]),
    "width-0": np.empty((2, 0), np.uint64),
    "width-129": np.tile(np.arange(129, dtype=np.uint64), (2, 1)),
    "not-2d": [3, 1, 2],
    "not-integers": [[3.0, 1.0, 2.0], [5.0, 4.0, 0.0]],
}


def _no_library(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("a library was loaded before the checks were done")
    monkeypatch.setattr(api, "load_library", fail)
    monkeypatch.setattr(api, "_predict_multiple", fail)


@pytest.mark.parametrize("case", sorted(BAD_LISTS))
def test_bad_lists_raise_before_the_device(monkeypatch, case):
    _no_library(monkeypatch)
    B = np.ones((NITEMS, K), np.float32)
    lists = BAD_LISTS[case] if isinstance(BAD_LISTS[case], np.ndarray) else np.array(BAD_LISTS[case], np.uint64 if case != "not-integers" else float)
    with pytest.raises(ValueError):
        api.list_eval(B, lists, item_norm=ONES)
    with pytest.raises(ValueError):
        _NoDeviceSession(True).list_eval(lists)
    with pytest.raises(ValueError):
        _fake_fitted(True).eval_lists(lists, users=[0, 1])
    with pytest.raises(ValueError):
        _NoDeviceSession(False).eval_lists(lists, users=[0, 1], item_norm=ONES)


def test_bad_norms_tests_and_budgets_raise_before_the_device(monkeypatch):
    _no_library(monkeypatch)
    B = np.ones((NITEMS, K), np.float64)
    lists = np.array(GOOD, np.uint64)
    for norm in ([-1.0] + ONES[1:], [np.nan] + ONES[1:], [np.inf] + ONES[1:], ONES[1:], np.ones((NITEMS, 2)), ["a"] * NITEMS):
        with pytest.raises(ValueError):
            api.list_eval(B, lists, item_norm=norm)
        with pytest.raises(ValueError):
            _fake_fitted(False).eval_lists(lists, users=[0, 1], item_norm=norm)
    for test in (([0, 2, 3], [4, 2, 1]), ([0, 2, 3], [2, 2, 1]), ([0, 1, 2], [1, NITEMS]), ([0, 1], [1]), ([0, 2, 1], [1, 2])):
        with pytest.raises(ValueError):
            api.list_eval(B, lists, test=test)
        with pytest.raises(ValueError):
            _NoDeviceSession(False).list_eval(lists, test=test)
    for budget in (0, -1, np.nan, "1", True, 1e-9, 2000 / 2 ** 20):      # the last: NITEMS x 12 B of norms and counts do not fit
        with pytest.raises(ValueError):
            api.list_eval(B, lists, budget_mb=budget)
    with pytest.raises(ValueError):
        api.list_eval(np.ones((NITEMS, 257)), lists)
    with pytest.raises(ValueError):
        api.list_eval(np.ones((NITEMS, K), np.float16), lists)


def test_eval_lists_arguments_raise_before_the_device(monkeypatch):
    _no_library(monkeypatch)
    model = _fake_fitted(True)
    lists = np.array(GOOD, np.uint64)
    X = sp.csr_matrix(([1.0, 1.0], ([0, 1], [3, 4])), shape=(NUSERS, NITEMS))
    for k in (0, 4, -1, 2.0, True):
        with pytest.raises(ValueError, match="k"):
            model.eval_lists(lists, users=[0, 1], k=k)
    for bad_X in (sp.csr_matrix((NUSERS, NITEMS + 1)), sp.csr_matrix((NUSERS + 1, NITEMS)), np.zeros((NUSERS, NITEMS))):
        with pytest.raises(ValueError, match="X_test"):
            model.eval_lists(lists, users=[0, 1], X_test=bad_X)
    with pytest.raises(ValueError, match="exclude"):
        model.eval_lists(lists, users=[0, 1], X_test=X, exclude=sp.csr_matrix((NUSERS, NITEMS + 1)))
    with pytest.raises(ValueError, match="exclude"):
        model.eval_lists(lists, users=[0, 1], exclude=X)
    for pop in (ONES[1:], np.ones((NITEMS, 1)), [-1.0] + ONES[1:], [np.nan] + ONES[1:], ["a"] * NITEMS):
        with pytest.raises(ValueError, match="item_pop"):
            model.eval_lists(lists, users=[0, 1], item_pop=pop)
    with pytest.raises(ValueError, match="users"):
        model.eval_lists(lists, users=[0, 1, 2])
    with pytest.raises(ValueError, match="out of range"):
        model.eval_lists(lists, users=[0, NUSERS])
    with pytest.raises(ValueError, match="one row per user"):
        model.eval_lists(lists, X_test=X)
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).eval_lists(lists)
    with pytest.raises(ValueError):
        _NoDeviceSession(True).eval_lists(lists, users=[0, 1], X_test=sp.csr_matrix((NUSERS, NITEMS + 1)))


def test_eval_lists_removes_excluded_cells_on_the_host():
    X = sp.csr_matrix(([1.0] * 5, ([0, 0, 0, 2, 3], [3, 4, 9, 4, 1])), shape=(NUSERS, NITEMS))
    E = sp.csr_matrix(([1.0] * 3, ([0, 2, 3], [4, 5, 1])), shape=(NUSERS, NITEMS))
    lists = np.array([[3, 1], [3, 1], [5, NONE], [9, 3]], np.uint64)
    out, test, pop = api._eval_lists_args(lists, [0, 3, 2, 0], X, 1, E, None, NUSERS, NITEMS)
    assert out.tolist() == [[3], [3], [5], [9]] and pop is None
    assert test[0].tolist() == [0, 2, 2, 3, 5] and test[1].tolist() == [3, 9, 4, 3, 9]
    assert test[0].dtype == np.uint64 and test[1].dtype == np.uint64
    pair = api._eval_lists_args(lists, [0, 3, 2, 0], X, None, ([0, 1, 2, 2, 3], [4, 1, 9]), None, NUSERS, NITEMS)[1]
    assert pair[0].tolist() == [0, 2, 2, 3, 5] and pair[1].tolist() == [3, 9, 4, 3, 4]


# ---- metrics.py ----
def test_metrics_from_positions_by_hand():
    A = api.LIST_ABSENT
    # user 0: held-out items at positions 0 and 2 and one absent; user 1: all absent; user 2: no cell; user 3: one at position 3
    indptr = [0, 3, 5, 5, 6]
    pos = [2, A, 0, A, A, 3]
    got = metrics.metrics_from_positions(indptr, pos, 4)
    assert sorted(got) == sorted(metrics.LIST_METRICS) and "auc" not in got
    l2 = np.log2
    ideal3 = 1 / l2(2) + 1 / l2(3) + 1 / l2(4)
    want = {
        "hit": [1, 0, np.nan, 1],
        "precision": [2 / 4, 0, np.nan, 1 / 4],
        "recall": [2 / 3, 0, np.nan, 1],
        "ap": [(1 / 1 + 2 / 3) / 3, 0, np.nan, (1 / 4) / 1],
        "ndcg": [(1 / l2(2) + 1 / l2(4)) / ideal3, 0, np.nan, (1 / l2(5)) / 1],
        "rr": [1, 0, np.nan, 1 / 4],
    }
    for name in metrics.LIST_METRICS:
        np.testing.assert_array_equal(got[name], np.array(want[name], np.float64), err_msg=name)
    means = metrics.mean_metrics(got, metrics.LIST_METRICS)
    assert means["n_users"] == 3 and means["hit"] == 2 / 3 and "auc" not in means
    with pytest.raises(ValueError):
        metrics.metrics_from_positions(indptr, pos, 3)                   # position 3 lies outside a list of three
    # lists of two: what was at positions 2 and 3 is absent now, and the cut-off is 2
    two = metrics.metrics_from_positions(indptr, [A, A, 0, A, A, A], 2)
    want2 = {"hit": [1, 0, np.nan, 0], "precision": [1 / 2, 0, np.nan, 0], "recall": [1 / 3, 0, np.nan, 0],
             "ap": [(1 / 1) / 2, 0, np.nan, 0], "ndcg": [(1 / l2(2)) / (1 / l2(2) + 1 / l2(3)), 0, np.nan, 0], "rr": [1, 0, np.nan, 0]}
    for name in metrics.LIST_METRICS:
        np.testing.assert_array_equal(two[name], np.array(want2[name], np.float64), err_msg=name)
    empty = metrics.metrics_from_positions([0], [], 5)
    assert all(len(empty[n]) == 0 for n in metrics.LIST_METRICS)


def test_ild_coverage_gini_novelty_by_hand():
    one = 2 ** 40
    got = metrics.ild(np.array([0, 0, one // 2, 3 * one, -one], np.int64), np.array([0, 1, 2, 3, 2], np.uint32))
    np.testing.assert_array_equal(got, [np.nan, np.nan, 0.5, 0.0, 2.0])
    assert metrics.coverage(np.array([0, 3, 0, 1], np.uint32)) == 0.5
    assert metrics.coverage(np.zeros(4, np.uint32)) == 0.0
    assert metrics.gini(np.array([2, 2, 2, 2], np.uint32)) == 0.0
    assert metrics.gini(np.array([0, 0, 0, 7], np.uint32)) == 3 / 4
    assert metrics.gini(np.array([3, 1, 0, 0], np.uint32)) == (-3 * 0 - 1 * 0 + 1 * 1 + 3 * 3) / (4 * 4)
    assert np.isnan(metrics.gini(np.zeros(5, np.uint32)))
    pop = np.array([8.0, 0.0, 4.0, 4.0])                     # sum 16; the unseen item counts as seen once
    lists = np.array([[0, 1], [2, NONE], [NONE, NONE], [3, 2]], np.uint64)
    np.testing.assert_array_equal(metrics.novelty(lists, pop), [(1 + 4) / 2, 2.0, np.nan, 2.0])
    assert metrics.nan_mean([np.nan, 1.0, 3.0]) == 2.0 and np.isnan(metrics.nan_mean([np.nan])) and np.isnan(metrics.nan_mean([]))


def test_the_result_dict(monkeypatch):
    """_lists_result on hand-made device outputs: the keys with and without X_test / item_pop / per_user"""
    lists = np.array([[0, 1], [2, NONE]], np.uint64)
    test = (np.array([0, 1, 1], np.uint64), np.array([1], np.uint64))
    pos, cos = np.array([1], np.uint32), np.array([2 ** 39, 0], np.int64)
    length, expo = np.array([2, 1], np.uint32), np.array([1, 1, 1, 0], np.uint32)
    out = api._lists_result(lists, test, pos, cos, length, expo, np.array([1.0, 1.0, 2.0, 0.0]), True)
    assert out["hit"] == 1.0 and out["rr"] == 0.5 and out["n_users"] == 1 and out["n_lists"] == 2
    assert out["ild"] == 0.5 and out["coverage"] == 0.75 and out["gini"] == metrics.gini(expo) and out["novelty"] == 1.5
    assert set(out["per_user"]) == set(metrics.LIST_METRICS) | {"ild", "novelty"}
    assert out["positions"] is pos and out["cos_sum"] is cos and out["length"] is length and out["exposure"] is expo
    assert out["test_indptr"] is test[0]
    out = api._lists_result(lists, None, None, cos, length, expo, None, False)
    assert set(out) == {"ild", "coverage", "gini", "n_users", "n_lists"} and out["n_users"] == 0
