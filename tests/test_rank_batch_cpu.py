"""CPU-side checks of the batched ranks' boundary (include/poismf_hip.h section 1g): the header declares the three prototypes with
the agreed parameter names and every library flavour exports them; metrics_from_ranks against a brute force written here from
the textbook definitions; every invalid input raises from PoisMF.eval_ranking, Session.eval_ranking and the raw rank_batch calls
before anything reaches a device; the C entry point itself answers 2 / 0 without one; and the one scratch allocation of a call
stays inside the budget the header states."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poismf_hip.h")
NAMES = ("poismf_hip_rank_batch", "poismf_hip_session_rank_batch", "poismf_hip_rank_batch_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def _params(name):
    text = open(HEADER).read()
    m = re.search(r"^POISMF_HIP_API\s+([\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text, re.M)
    assert m, f"{name} is not declared"
    return " ".join(m.group(1).split()), [re.match(r".*?(\w+)$", " ".join(p.split())).group(1) for p in m.group(2).split(",")]


def _define(name):
    m = re.search(r"^#define\s+" + name + r"\s+(0x[0-9a-fA-F]+|\d+)", open(HEADER).read(), re.M)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1), 0)


# ---- 1. the boundary --------------------------------------------------------------------------------------------------------------

def test_header_declares_the_prototypes():
    ret, names = _params("poismf_hip_rank_batch")
    assert ret == "int"
    assert names == ["A", "B", "k", "dimA", "dimB", "users", "n_users", "test_indptr", "test_indices", "excl_indptr", "excl_indices",
                     "out_rank", "out_n_adm"]
    ret, names = _params("poismf_hip_session_rank_batch")
    assert ret == "int"
    assert names == ["s", "users", "n_users", "test_indptr", "test_indices", "exclude_seen", "excl_indptr", "excl_indices", "out_rank",
                     "out_n_adm"]
    ret, names = _params("poismf_hip_rank_batch_scratch_bytes")
    assert ret == "size_t" and names == ["n_users", "n_cells", "dimB", "k"]
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_RANK_EXCLUDED") == 0xFFFFFFFF == api.RANK_EXCLUDED == metrics.RANK_EXCLUDED
    assert _define("POISMF_HIP_RANK_BATCH_MAX_ROW") == api.RANK_BATCH_MAX_ROW
    assert _define("POISMF_HIP_RANK_BATCH_BUDGET_MB") == api.RANK_BATCH_BUDGET_MB


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_rank_batch(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


# ---- 2. the metrics against a brute force -------------------------------------------------------------------------------------------

def _brute(scores, excluded, held_out, K):
    """One user, from the textbook: the ranked list of the admissible items, walked from the top.  Returns (ranks in held_out's
    order with RANK_EXCLUDED for excluded cells, N, dict of the seven metrics or None when no held-out cell is admissible)."""
    n = len(scores)
    adm = np.setdiff1d(np.arange(n), np.asarray(excluded, np.int64))
    ranked = adm[np.lexsort((adm, -scores[adm]))]             # score descending, item ascending
    place = {int(j): pos for pos, j in enumerate(ranked)}
    ranks = np.array([place.get(int(t), metrics.RANK_EXCLUDED) for t in held_out], np.int64)
    positives = {int(t) for t in held_out if int(t) in place}
    N, p = len(ranked), len(positives)
    if p == 0:
        return ranks, N, None
    hits, dcg, ap_sum, first = 0, 0.0, 0.0, None
    for pos, j in enumerate(ranked[:K]):
        if int(j) in positives:
            hits += 1
            ap_sum += hits / (pos + 1)                          # precision at this position
            dcg += 1.0 / math.log2(pos + 2)
            if first is None:
                first = pos
    ideal = sum(1.0 / math.log2(i + 2) for i in range(min(K, p)))
    # AUC: the share of (positive, negative) pairs of admissible items in which the positive stands first
    is_pos = np.array([int(j) in positives for j in ranked])
    negatives_after = np.cumsum((~is_pos)[::-1])[::-1]
    right = int(negatives_after[is_pos].sum())
    out = {
        "hit": 1.0 if hits else 0.0,
        "precision": hits / K,
        "recall": hits / p,
        "ap": ap_sum / min(K, p),
        "ndcg": dcg / ideal,
        "rr": 1.0 / (first + 1) if first is not None else 0.0,
        "auc": right / (p * (N - p)) if N > p else float("nan"),
    }
    return ranks, N, out


def _metric_case(rng, n_items, tied):
    """(scores, excluded, held_out) of one user"""
    scores = rng.integers(0, 4, n_items).astype(np.float64) if tied else rng.random(n_items)
    excluded = np.sort(rng.choice(n_items, int(rng.integers(0, n_items // 2 + 1)), replace=False))
    held_out = np.sort(rng.choice(n_items, int(rng.integers(0, n_items + 1)), replace=False))
    return scores, excluded, held_out


@pytest.mark.parametrize("tied", [False, True], ids=["random", "tied"])
def test_metrics_against_brute_force(tied):
    """bound 1e-12 absolute: each metric is a sum of at most max(K, p) float64 terms of size at most 1, so two ways of adding them
    differ by a few units of 2^-53 per term"""
    rng = np.random.default_rng(11 + tied)
    worst = 0.0
    for trial in range(150):
        n_items = int(rng.integers(1, 60))
        m = int(rng.integers(1, 9))
        users = [_metric_case(rng, n_items, tied) for _ in range(m)]
        if trial % 10 == 0:                                     # a user whose every held-out cell is excluded, one with none,
            sc = rng.random(n_items)                            # and one whose held-out cells are all the admissible items (N == p)
            users.append((sc, np.arange(n_items), np.arange(n_items)))
            users.append((sc, np.empty(0, np.int64), np.empty(0, np.int64)))
            excl = np.arange(n_items // 2)
            users.append((sc, excl, np.arange(n_items)))
        for K in sorted({1, 2, 3, 10, n_items, n_items + 5}):
            indptr, ranks, n_adm, want = [0], [], [], []
            for scores, excluded, held_out in users:
                r, N, mt = _brute(scores, excluded, held_out, K)
                order = rng.permutation(len(r))                 # (the ranks of a row may come in any order)
                ranks.extend(r[order].tolist())
                indptr.append(len(ranks))
                n_adm.append(N)
                want.append(mt)
            got = metrics.metrics_from_ranks(np.array(indptr), np.array(ranks, np.uint32), np.array(n_adm, np.uint32), K)
            for i, mt in enumerate(want):
                for name in metrics.METRICS:
                    g = got[name][i]
                    if mt is None or math.isnan(mt[name]):
                        assert math.isnan(g), (trial, K, i, name, g)
                    else:
                        worst = max(worst, abs(g - mt[name]))
                        assert abs(g - mt[name]) <= 1e-12, (trial, K, i, name, g, mt[name])
            means = metrics.mean_metrics(got)
            counted = [mt for mt in want if mt is not None]
            assert means["n_users"] == len(counted)
            for name in metrics.METRICS:
                vals = [mt[name] for mt in counted if not math.isnan(mt[name])]
                if vals:
                    assert abs(means[name] - float(np.mean(vals))) <= 1e-12
                else:
                    assert math.isnan(means[name])
    print(f"largest difference to the brute force: {worst:.3g}")


def test_metrics_hand_checked():
    """one user by hand: ranks 0 and 5 of 10 admissible items, cut-off 3"""
    got = metrics.metrics_from_ranks([0, 3], np.array([5, 0xFFFFFFFF, 0], np.uint32), [10], 3)
    assert got["hit"][0] == 1 and got["rr"][0] == 1
    assert got["precision"][0] == pytest.approx(1 / 3, abs=1e-15) and got["recall"][0] == 0.5 and got["ap"][0] == 0.5
    assert got["ndcg"][0] == pytest.approx(1 / (1 + 1 / math.log2(3)), abs=1e-15)
    assert got["auc"][0] == 1 - 4 / 16                       # the held-out item at rank 5 has 4 others before it; 2 x 8 pairs
    with pytest.raises(ValueError):
        metrics.metrics_from_ranks([0, 1], [0], [5], 0)
    with pytest.raises(ValueError):
        metrics.metrics_from_ranks([0, 2], [0], [5], 1)


# ---- 3. invalid input ----------------------------------------------------------------------------------------------------------------

NUSERS, NITEMS, K = 6, 300, 3


def _fake_fitted(use_float):
    """a model that looks fitted without any fit having run (no device is touched)"""
    m = api.PoisMF(k=K, use_float=use_float)
    dt = np.float32 if use_float else np.float64
    m.A, m.B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    m.nusers, m.nitems = NUSERS, NITEMS
    m.is_fitted = True
    return m


class _NoDeviceSession(api.Session):
    """the Python half of a session, never connected to a device: any library call would fail on the missing handle"""

    def __init__(self, use_float):
        self.lib = None
        self.use_float = use_float
        self.dimA, self.dimB, self.k = NUSERS, NITEMS, K
        self.shardA, self.shardB = (0, 4), (0, NITEMS)
        self.h = None


def _x(rows, cols, shape=(NUSERS, NITEMS)):
    return sp.csr_matrix((np.ones(len(rows)), (np.asarray(rows), np.asarray(cols))), shape=shape)


X_OK = _x([0, 1, 1], [5, 7, 9])
# eval_ranking(X_test, k, exclude, users): every one invalid
BAD_EVAL = {
    "user-out-of-range": (X_OK, 5, None, [0, NUSERS]),
    "negative-user": (X_OK, 5, None, [-1, 0]),
    "k-zero": (X_OK, 0, None, None),
    "k-negative": (X_OK, -3, None, None),
    "test-more-columns": (_x([0], [5], (NUSERS, NITEMS + 1)), 5, None, None),
    "test-fewer-rows": (_x([0], [5], (NUSERS - 1, NITEMS)), 5, None, None),
    "test-not-sparse": (np.ones((NUSERS, NITEMS)), 5, None, None),
    "exclude-wrong-shape": (X_OK, 5, _x([0], [5], (NUSERS, NITEMS - 1)), None),
    "exclude-item-out-of-range": (X_OK, 5, ([0, 1, 2], [3, NITEMS]), [0, 1]),
    "exclude-negative-item": (X_OK, 5, ([0, 1, 2], [-2, 4]), [0, 1]),
    "exclude-descending-row": (X_OK, 5, ([0, 2, 4], [1, 2, 9, 7]), [0, 1]),
    "exclude-repeated-item": (X_OK, 5, ([0, 2, 4], [1, 2, 7, 7]), [0, 1]),
    "exclude-wrong-rows": (X_OK, 5, ([0, 1, 2, 3], [1, 2, 3]), [0, 1]),
    "exclude-decreasing-indptr": (X_OK, 5, ([0, 2, 1], [1, 2]), [0, 1]),
}


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD_EVAL))
def test_eval_ranking_raises_before_the_device(use_float, case):
    X, k, excl, users = BAD_EVAL[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).eval_ranking(X, k=k, exclude=excl, users=users)


@pytest.mark.parametrize("case", sorted(BAD_EVAL))
def test_session_eval_ranking_raises_before_the_device(case):
    X, k, excl, users = BAD_EVAL[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).eval_ranking(X, k=k, exclude=excl, users=users, exclude_seen=False)


def test_eval_ranking_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).eval_ranking(X_OK)


def test_session_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).eval_ranking(_x([1, 5], [3, 4]), exclude_seen=True)      # (user 5 is outside rows 0..3)
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).rank_batch([1, 5], ([0, 1, 2], [3, 4]), exclude_seen=True)


# the raw calls: (users, test as (indptr, indices), exclude as (indptr, indices) or None): every one invalid
BAD = {
    "user-out-of-range": ([0, NUSERS], ([0, 1, 2], [3, 4]), None),
    "negative-user": ([-1, 0], ([0, 1, 2], [3, 4]), None),
    "test-item-out-of-range": ([0, 1], ([0, 1, 2], [3, NITEMS]), None),
    "test-negative-item": ([0, 1], ([0, 1, 2], [-2, 4]), None),
    "test-descending-row": ([0, 1], ([0, 2, 4], [1, 2, 9, 7]), None),
    "test-repeated-item": ([0, 1], ([0, 2, 4], [1, 2, 7, 7]), None),
    "test-decreasing-indptr": ([0, 1], ([0, 2, 1], [1, 2]), None),
    "test-wrong-rows": ([0, 1], ([0, 1, 2, 3], [1, 2, 3]), None),
    "exclude-item-out-of-range": ([0, 1], ([0, 1, 2], [3, 4]), ([0, 1, 2], [3, NITEMS])),
    "exclude-negative-item": ([0, 1], ([0, 1, 2], [3, 4]), ([0, 1, 2], [-2, 4])),
    "exclude-descending-row": ([0, 1], ([0, 1, 2], [3, 4]), ([0, 2, 4], [1, 2, 9, 7])),
    "exclude-repeated-item": ([0, 1], ([0, 1, 2], [3, 4]), ([0, 2, 4], [1, 2, 7, 7])),
    "exclude-wrong-rows": ([0, 1], ([0, 1, 2], [3, 4]), ([0, 1, 2, 3], [1, 2, 3])),
}
NO_ROW_COUNT = {"test-wrong-rows", "exclude-wrong-rows"}   # (a C caller has no row count to get wrong)


@pytest.mark.parametrize("case", sorted(BAD))
def test_raw_wrappers_raise_before_the_device(case):
    users, test, excl = BAD[case]
    with pytest.raises(ValueError):
        _NoDeviceSession(True).rank_batch(users, test, exclude=excl)
    for dt in (np.float32, np.float64):
        with pytest.raises(ValueError):
            api.rank_batch(np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt), users, test, exclude=excl)


def test_raw_wrapper_row_too_long():
    long_row = np.arange(api.RANK_BATCH_MAX_ROW + 1)
    B = np.ones((len(long_row), 2), np.float32)
    with pytest.raises(ValueError, match="longer"):
        api.rank_batch(np.ones((2, 2), np.float32), B, [0], ([0, len(long_row)], long_row))


def _c_call(flavour, users, test, excl, n_users=None, k=K):
    """poismf_hip_rank_batch itself through ctypes; index arrays in the flavour's sparse_ix"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, max(k, 1)), dt), np.ones((NITEMS, max(k, 1)), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    tp, ti = ix(test[0]), ix(test[1])
    rank = np.full(max(len(ti), 1), 12345, np.uint32)
    n_adm = np.full(max(m, 1), 54321, np.uint32)
    p = api._ptr
    ep, ei = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    rc = lib.poismf_hip_rank_batch(p(A), p(B), k, NUSERS, NITEMS, p(u), m, p(tp), p(ti), p(ep) if ep is not None else None,
                                   p(ei) if ei is not None else None, p(rank), p(n_adm))
    return rc, rank, n_adm


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_returns_2_and_writes_nothing(flavour, case):
    users, test, excl = BAD[case]
    rc, rank, n_adm = _c_call(flavour, users, test, excl)
    assert rc == 2
    assert np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_no_users_is_not_an_error(flavour):
    rc, rank, n_adm = _c_call(flavour, [0], ([0, 1], [3]), None, n_users=0)
    assert rc == 0 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour,kmax", [(False, 256), (True, 512), ("r", 256)], ids=["d", "f", "r"])
def test_c_entry_k_out_of_range(flavour, kmax):
    for k in (0, -1, kmax + 1):
        rc, rank, n_adm = _c_call(flavour, [0, 1], ([0, 1, 2], [3, 4]), None, k=k)
        assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


def test_c_entry_row_too_long():
    lib = api.load_library(True)
    n = api.RANK_BATCH_MAX_ROW + 1
    A, B = np.ones((1, 2), np.float32), np.ones((n, 2), np.float32)
    u, tp, ti = np.zeros(1, np.uint64), np.array([0, n], np.uint64), np.arange(n, dtype=np.uint64)
    rank, n_adm = np.full(n, 12345, np.uint32), np.full(1, 54321, np.uint32)
    p = api._ptr
    assert lib.poismf_hip_rank_batch(p(A), p(B), 2, 1, n, p(u), 1, p(tp), p(ti), None, None, p(rank), p(n_adm)) == 2
    assert np.all(rank == 12345) and np.all(n_adm == 54321)


# ---- 4. the scratch ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_stated_budget(flavour):
    """the size both entry points allocate (one allocation per call), against the figure in the header's own text"""
    budget = _define("POISMF_HIP_RANK_BATCH_BUDGET_MB") << 20
    fn = api.load_library(flavour).poismf_hip_rank_batch_scratch_bytes
    kmax = 512 if flavour else 256
    users = sorted({1, 2, 63, 64, 65, 1000, 4096, 10 ** 5, 10 ** 6, 10 ** 7} | {int(x) for x in np.logspace(0, 7, 40)})
    per_user = [0, 1, 2, 10, 31, 32, 33, 100, 1000, 10 ** 4]
    items = sorted({1, 2, 64, 1000, 25000, 10 ** 5, 10 ** 6, 2 ** 31 - 1})
    worst = 0
    for m in users:
        for c in per_user:
            for dimB in items:
                for k in (1, 50, kmax):
                    b = int(fn(m, m * c, dimB, k))
                    assert 0 < b <= budget, (m, c, dimB, k, b)
                    worst = max(worst, b)
    # a small call does not pay for a large one
    assert int(fn(64, 640, 1000, 50)) < (8 << 20)
    assert worst > (budget >> 2)   # (the bound is not vacuous: large calls do use a good part of it)
