"""Sampled ranks in one pass (include/poismf_hip.h section 1u) on the GPU against a reference that holds no GPU code: the sample is
tests/test_gpu_sample_negatives.py's Philox in Python integers with the header's sequential rule, the scores are a float64 product and
the order is a lexsort.  The factors are small non-negative integers (times a power of two), so every fused chain is exact in float32
and float64 alike and ties are frequent: ranks, n_adm, count and draws are compared as integers, with no tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests.serving_values import _csr_pair
from tests.test_gpu_sample_negatives import lists, reference

pytestmark = pytest.mark.gpu

DIMA, DIMB = 8, 70000
HELD = (0, 1, 128, 129, 7, 3, 40, 2)      # held-out row lengths by user: none, one, the LDS group of 128 full, and one past it
W7 = 1 + np.arange(DIMB) % 7
BASE = dict(dimB=DIMB, m=64, k=50, dt=np.float32, mode="none", weight=None, users=(1, 6, 3, 2, 1), scale=1.0, seed=11)
MODES = ("none", "list", "seen", "both")
CASES = {
    # m at the round edges (63, 64, 65), the instance edge (256, 257) and the limits, the exclusion modes in turn
    **{f"m{m}-{MODES[i % 4]}": dict(m=m, mode=MODES[i % 4], seed=99 + m) for i, m in enumerate((1, 63, 64, 65, 256, 257, 1000, 4096))},
    **{f"m{m}-{mode}": dict(m=m, mode=mode) for m in (64, 257) for mode in MODES if f"m{m}-{mode}" not in ("m64-seen", "m257-list")},
    "in-round-duplicates": dict(dimB=8, m=8, users=(3, 0), seed=12345),
    "cap-bites": dict(dimB=97, m=64, mode="evens", users=(3, 5, 0), seed=3),
    "all-excluded": dict(dimB=97, m=5, mode="all", users=(2, 4)),
    # k = 1, the serving default, two chunks of columns, and either side of tb_gather's column chunk (64 floats, 32 doubles)
    **{f"f32-k{k}": dict(k=k, m=65, mode="list", scale=0.25) for k in (1, 63, 64, 65, 100)},
    **{f"f64-k{k}": dict(k=k, m=65, mode="list", dt=np.float64) for k in (1, 31, 32, 33, 50, 100)},
    "f64-seen-m300": dict(m=300, mode="both", dt=np.float64, scale=4.0),
    "weight-zeros": dict(dimB=50, m=10, weight=np.where(np.arange(50) % 3 == 0, 0, np.arange(50) * 1000 + 1), users=(5, 0, 5)),
    "weight-coarse-small": dict(m=64, mode="both", weight=W7),
    "weight-coarse-big": dict(m=300, mode="list", weight=W7, users=(7, 2, 7)),
}


@pytest.fixture(scope="module")
def sessions():
    """sessions of DIMA users whose seen rows hold about a third of the items, made on first use per precision"""
    rng = np.random.default_rng(7)
    seen = [np.sort(rng.choice(DIMB, DIMB // 3, replace=False)) for _ in range(DIMA)]
    rows = np.concatenate([np.full(len(s), u) for u, s in enumerate(seen)])
    X = sp.coo_matrix((np.ones(len(rows)), (rows, np.concatenate(seen))), shape=(DIMA, DIMB))
    made = {}
    yield seen, lambda dt: made.get(dt) or made.setdefault(dt, api.Session.from_coo(X, 50, dt == np.float32))
    for s in made.values():
        s.close()


def expected(A, B, u, seed, m, E, T, weight):
    """section 1u's definition for one user: (ranks of T's cells, N(u), |S(u)|, draws)"""
    S, draws = reference(seed, u, m, B.shape[0], np.union1d(E, T), weight)
    C = np.union1d(S, np.setdiff1d(T, E)).astype(np.int64)
    scores = A[u].astype(np.float64) @ B[C].astype(np.float64).T
    order = C[np.lexsort((C, -scores))]
    place = {int(j): r for r, j in enumerate(order)}
    return [place.get(int(t), api.RANK_EXCLUDED) for t in T], len(C), len(S), draws


@pytest.mark.parametrize("case", sorted(CASES))
def test_ranks_equal_the_definition(sessions, case):
    c = {**BASE, **CASES[case]}
    dimB, m, k, dt, mode, users = c["dimB"], c["m"], c["k"], c["dt"], c["mode"], list(c["users"])
    seen, session = sessions
    rng = np.random.default_rng(k + m)
    A, B = (rng.integers(0, 4, (DIMA, k)) * c["scale"]).astype(dt), rng.integers(0, 4, (dimB, k)).astype(dt)
    excl = {"none": None, "evens": [np.arange(0, dimB, 2)] * len(users), "all": [np.arange(dimB)] * len(users)}.get(mode) or (
        lists(users, dimB) if mode in ("list", "both") else None)
    # held-out rows: HELD[u] items; where there is an exclusion list every second row takes its first two cells from it, and the
    # last user's row lies wholly inside it
    held = [np.sort(rng.choice(dimB, min(HELD[u], dimB // 2), replace=False)) for u in users]
    if excl:
        held = [np.union1d(h[2:], excl[i][:2]) if i % 2 and len(h) else h for i, h in enumerate(held)]
        held[-1] = excl[-1][:3]
    kw = dict(exclude=_csr_pair(excl) if excl else None, item_weight=c["weight"], seed=c["seed"], return_counts=True)
    if mode in ("seen", "both"):
        s = session(dt)
        s.set_factors(A, B)
        ranks, n_adm, count, draws = s.rank_sampled(users, _csr_pair(held), m, exclude_seen=True, **kw)
    else:
        ranks, n_adm, count, draws = api.rank_sampled(A, B, users, _csr_pair(held), m, **kw)
    at = np.concatenate(([0], np.cumsum([len(h) for h in held])))
    for i, u in enumerate(users):
        E = np.union1d(excl[i] if excl else [], seen[u] if mode in ("seen", "both") else [])
        want = expected(A, B, u, c["seed"], m, E, held[i], c["weight"])
        got = (ranks[at[i]:at[i + 1]].tolist(), int(n_adm[i]), int(count[i]), int(draws[i]))
        print(case, "user", u, "cells", len(held[i]), "n_adm, count, draws", got[1:], "reference", want[1:])
        assert got == want
    if case == "cap-bites":
        assert np.all(count < m) and np.all(draws == 16 * m + 256)
    if case == "all-excluded":
        assert not n_adm.any() and np.all(ranks == api.RANK_EXCLUDED)


def test_a_row_depends_on_its_own_inputs_only():
    """another order of the batch, and the other side of the chunk cut (262144 users): the same rows"""
    n, k = 262144 + 3, 2
    rng = np.random.default_rng(5)
    A, B = rng.integers(0, 4, (n, k)).astype(np.float32), rng.integers(0, 4, (1000, k)).astype(np.float32)
    first = rng.integers(0, 250, (n, 2)).astype(np.uint64) * 2             # two cells per user: an even item, then a larger odd one
    held = (np.arange(n + 1, dtype=np.uint64) * 2, np.stack((first[:, 0], first[:, 0] + first[:, 1] + 1), axis=1).reshape(-1))
    whole = api.rank_sampled(A, B, np.arange(n), held, 5, seed=2, return_counts=True)
    pick = np.array([n - 1, 7, n - 3, 262143, 7])                          # out of order, one user twice, from both chunks
    cells = (np.arange(len(pick) + 1) * 2, np.concatenate([held[1][2 * u:2 * u + 2] for u in pick]))
    few = api.rank_sampled(A, B, pick, cells, 5, seed=2, return_counts=True)
    assert np.array_equal(few[0].reshape(-1, 2), whole[0].reshape(-1, 2)[pick])
    for a, b in zip(few[1:], whole[1:]):
        assert np.array_equal(a, b[pick])
    assert np.all(whole[1] == 7) and np.all(whole[2] == 5)
