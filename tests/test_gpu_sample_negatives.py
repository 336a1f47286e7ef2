"""Sampled negatives (include/poismf_hip.h section 1t) on the GPU against a reference that holds no GPU code: Philox4x32-10 in Python
integers and the header's sequential rule.  Items, counts and draws are compared for equality; there is no tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests.serving_values import _csr_pair

pytestmark = pytest.mark.gpu

MASK, DIMA, DIMB = 2 ** 32 - 1, 8, 70000


def philox(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + 0x9E3779B9) & MASK, (k[1] + 0xBB67AE85) & MASK]
    return c


def reference(seed, u, m, dimB, excluded, weight):
    """the header's rule for one user: (accepted items ascending, draws consumed)"""
    C = None if weight is None else np.cumsum(np.asarray(weight, np.uint64), dtype=np.uint64)
    excluded, taken, cap = set(int(j) for j in excluded), set(), 16 * m + 256
    for d in range(cap):
        w = philox((d, 0, u & MASK, u >> 32), (seed & MASK, seed >> 32))
        r = (w[1] << 32) | w[0]
        if C is None:
            j = (r * dimB) >> 64
        else:
            j = int(np.searchsorted(C, np.uint64((r * int(C[-1])) >> 64), side="right"))   # the first item with C_j > t
        if j not in excluded and j not in taken:
            taken.add(j)
            if len(taken) == m:
                return sorted(taken), d + 1
    return sorted(taken), cap


@pytest.fixture(scope="module")
def world():
    """a session of DIMA users whose seen rows hold about a third of the items, the held-out cells, and factors"""
    rng = np.random.default_rng(7)
    seen = [np.sort(rng.choice(DIMB, DIMB // 3, replace=False)) for _ in range(DIMA)]
    rows = np.concatenate([np.full(len(s), u) for u, s in enumerate(seen)])
    s = api.Session.from_coo(sp.coo_matrix((np.ones(len(rows)), (rows, np.concatenate(seen))), shape=(DIMA, DIMB)), 4, True)
    s.set_factors(rng.random((DIMA, 4), np.float32), rng.random((DIMB, 4), np.float32))
    yield s, seen
    s.close()


def lists(users, dimB, seed=1):
    """a batch exclusion list per user: every third item or so"""
    return [np.flatnonzero(np.random.default_rng(seed + int(u) % 1000).random(dimB) < 0.3) for u in users]


BIG = [5, 2 ** 32 + 5, 2 ** 40 + 1]          # host flavour: ids that differ only in the counter's fourth word
W7 = 1 + np.arange(DIMB) % 7
SPARSE_W = np.where(np.arange(50) % 3 == 0, 0, np.arange(50) * 1000 + 1)
HEAVY_W = np.where(np.isin(np.arange(100), (7, 40, 99)), 10 ** 6, 1)
# id: (dimB, m, users, seed, mode, weight)
CASES = {
    "in-round-duplicates": (8, 8, [3], 12345, "none", None),
    "short-row": (97, 64, [0, 11], 3, "evens", None),
    "all-excluded": (97, 5, [2, 4], 3, "all", None),
    **{f"m{m}-{mode}": (DIMB, m, BIG[:2] if mode in ("none", "list") else [1, 6], 99 + m, mode, None)
       for m in (1, 63, 64, 65, 256, 257, 1000, 4096) for mode in ("none", "list", "seen", "both")},
    "weight-zeros": (50, 10, BIG, 5, "none", SPARSE_W),
    "weight-heavy": (100, 5, BIG, 6, "none", HEAVY_W),
    "weight-coarse-small": (DIMB, 64, [2, 3], 8, "both", W7),
    "weight-coarse-big": (DIMB, 300, BIG[1:], 8, "list", W7),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_equal_the_sequential_rule(world, case):
    dimB, m, users, seed, mode, weight = CASES[case]
    s, seen = world
    excl = {"none": None, "evens": [np.arange(0, dimB, 2)] * len(users), "all": [np.arange(dimB)] * len(users)}.get(mode) or (
        lists(users, dimB) if mode in ("list", "both") else None)
    kw = dict(exclude=_csr_pair(excl) if excl else None, item_weight=weight, seed=seed, return_draws=True)
    if mode in ("seen", "both"):
        indptr, items, draws = s.sample_negatives(users, m, exclude_seen=True, **kw)
    else:
        indptr, items, draws = api.sample_negatives(dimB, np.asarray(users, np.uint64), m, **kw)
    for i, u in enumerate(users):
        E = np.union1d(excl[i] if excl else [], seen[u] if mode in ("seen", "both") else [])
        want, want_draws = reference(seed, u, m, dimB, E, weight)
        got = items[indptr[i]:indptr[i + 1]]
        print(case, u, "count", len(got), "draws", int(draws[i]), "reference", len(want), want_draws)
        assert got.tolist() == want and int(draws[i]) == want_draws
    if case == "in-round-duplicates":
        assert draws[0] == 19
    if case == "short-row":
        assert np.all(np.diff(indptr) == 48) and np.all(draws == 16 * 64 + 256)
    if case == "all-excluded":
        assert indptr[-1] == 0
    if weight is not None:
        assert np.all(np.asarray(weight)[items.astype(np.int64)] > 0)


def rows(out):
    return [out[1][a:b].tolist() for a, b in zip(out[0][:-1], out[0][1:])]


def test_a_row_depends_on_its_own_inputs_only():
    alone = rows(api.sample_negatives(DIMB, [41], 65, seed=9))[0]
    batch = np.r_[np.arange(100, 250), 41, np.arange(300, 448), 41].astype(np.uint64)      # 300 users, user 41 twice
    got = rows(api.sample_negatives(DIMB, batch, 65, seed=9))
    assert got[150] == alone and got[299] == alone and got[0] != alone
    assert set(rows(api.sample_negatives(DIMB, [41], 63, seed=9))[0]) < set(alone)
    # either side of the chunk cut (262144 users): the last users' rows are those of the users alone
    for n in (262144, 262145):
        got = api.sample_negatives(1000, np.arange(n, dtype=np.uint64), 1, seed=2)
        assert len(got[1]) == n
        for u in (n - 2, n - 1):
            assert got[1][u] == api.sample_negatives(1000, [u], 1, seed=2)[1][0] == reference(2, u, 1, 1000, (), None)[0][0]


def test_eval_ranking_draws_the_sample_it_is_given(world):
    s, seen = world
    rng = np.random.default_rng(3)
    held = [np.setdiff1d(rng.choice(DIMB, 20, replace=False), seen[u]) for u in range(DIMA)]
    held[2] = held[2][:0]                                                                 # a user without held-out cells is not evaluated
    r = np.concatenate([np.full(len(h), u) for u, h in enumerate(held)])
    X_test = sp.csr_matrix((np.ones(len(r)), (r, np.concatenate(held))), shape=(DIMA, DIMB))
    users = np.flatnonzero(np.diff(X_test.indptr))
    sample = s.sample_negatives(users, 50, exclude_seen=True, exclude=_csr_pair([held[u] for u in users]), seed=77)
    assert np.all(np.diff(sample[0]) == 50)
    a, b = s.eval_ranking(X_test, negatives=50, seed=77, per_user=True), s.eval_ranking(X_test, include=sample, per_user=True)
    assert np.array_equal(a["ranks"], b["ranks"]) and np.array_equal(a["n_adm"], b["n_adm"]) and np.all(a["n_adm"] == 50 + np.diff(X_test.indptr)[users])
    assert {k: v for k, v in a.items() if np.isscalar(v)} == {k: v for k, v in b.items() if np.isscalar(v)}
