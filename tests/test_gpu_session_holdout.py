"""Session.holdout / api.holdout_split (include/poismf_hip.h section 2f) against the rule written out in numpy: Philox keys from the sampler
test's own generator, a lexsort by (key, item) per row, the first h(u) cells.  Everything is compared as integers or bits.  One small matrix
whose row lengths sit on every boundary of the selection's tiers (256 cells a wave holds, 4096 a workgroup's LDS holds).  Needs an MI355X."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests.test_gpu_sample_negatives import MASK, philox

pytestmark = pytest.mark.gpu

DIMB, SEED, MAX = 12000, 0x9E3779B97F4A7C15, 2 ** 64 - 1
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 700, 4095, 4096, 4097, 9000, 0, 130, 5, 1]
RULES = [(1, 2 ** 32, 1), (5, 2 ** 32, 0), (MAX, 2 ** 31, 3), (MAX, 0, 0), (MAX, 2 ** 32, 0)]   # (n_out, thresh, min_keep)
FRAC = {2 ** 32: 1.0, 2 ** 31: 0.5, 0: 0.0}                                                     # the wrapper's frac for each thresh


@pytest.fixture(scope="module")
def problem():
    """(X, key per stored cell): values are small dyadic numbers, the same in both precisions"""
    rng = np.random.default_rng(5)
    rows = [np.sort(rng.choice(DIMB, n, replace=False)) for n in LENGTHS]
    indptr = np.concatenate([[0], np.cumsum(LENGTHS)])
    X = sp.csr_matrix((rng.integers(1, 64, indptr[-1]) / 4.0, np.concatenate(rows), indptr), shape=(len(LENGTHS), DIMB))
    keys = np.empty(X.nnz, np.uint64)
    for u in range(X.shape[0]):
        for p in range(X.indptr[u], X.indptr[u + 1]):
            w = philox((int(X.indices[p]), 1, u & MASK, u >> 32), (SEED & MASK, SEED >> 32))
            keys[p] = (w[0] << 32) | w[1]
    return X, keys


def reference(problem, rule, users=None):
    """the held-out cells of `users` as a CSR over them: section 2f's rule, row by row"""
    (X, keys), (n_out, thresh, min_keep) = problem, rule
    users = range(X.shape[0]) if users is None else users
    indptr, taken = [0], []
    for u in users:
        lo, hi = X.indptr[u], X.indptr[u + 1]
        below = int(((keys[lo:hi] >> np.uint64(32)).astype(np.int64) < thresh).sum())
        h = min(n_out, below, max(hi - lo - min_keep, 0))
        taken.append(lo + np.sort(np.lexsort((X.indices[lo:hi], keys[lo:hi]))[:h]))
        indptr.append(indptr[-1] + h)
    taken = np.concatenate(taken).astype(np.int64)
    return sp.csr_matrix((X.data[taken], X.indices[taken], indptr), shape=(len(indptr) - 1, X.shape[1]))


def same_csr(got, want, dt):
    assert got.shape == want.shape and got.dtype == dt
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint8), want.data.astype(dt).view(np.uint8))


def session(X, prec, k=4):
    return api.Session.from_coo(X.tocoo(), k, prec)


def holdout(s, rule, **kw):
    n_out, thresh, min_keep = rule
    return s.holdout(None if n_out == MAX else n_out, FRAC[thresh], min_keep, SEED, **kw)


@pytest.mark.parametrize("prec", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("rule", RULES, ids=["leave1", "leave5", "half_keep3", "none", "all"])
def test_the_split_is_the_rule_s_and_the_session_becomes_the_training_matrix(problem, rule, prec):
    X, dt = problem[0], np.float32 if prec else np.float64
    want = reference(problem, rule)
    assert want.nnz == {RULES[3]: 0, RULES[4]: X.nnz}.get(rule, want.nnz) and (rule in RULES[3:] or 0 < want.nnz < X.nnz)
    s = session(X, prec)
    before = [s.matrix(w) for w in (0, 1)]
    same_csr(holdout(s, rule, remove=False), want, dt)
    for w in (0, 1):
        assert all(np.array_equal(a, b) for a, b in zip(s.matrix(w), before[w]))
    same_csr(holdout(s, rule), want, dt)
    train = (X - want).tocsr()
    train.eliminate_zeros()
    assert s.nnz(1) == s.nnz(0) == train.nnz == X.nnz - want.nnz
    if train.nnz:
        fresh = session(train, prec)
        for w in (0, 1):
            for got, exp in zip(s.matrix(w), fresh.matrix(w)):
                assert got.dtype == exp.dtype and np.array_equal(got.view(np.uint8), exp.view(np.uint8))
        fresh.close()
    s.close()


@pytest.mark.parametrize("rule", [RULES[1], RULES[2]], ids=["leave5", "half_keep3"])
def test_a_row_does_not_depend_on_the_users_it_is_listed_with(problem, rule):
    s = session(problem[0], True)
    for users in ([15], [13], np.random.default_rng(1).permutation(len(LENGTHS))[:14], [14, 9, 15, 0, 12]):
        same_csr(holdout(s, rule, users=users, remove=False), reference(problem, rule, users), np.float32)
    s.close()


@pytest.mark.parametrize("rule", [RULES[0], RULES[2]], ids=["leave1", "half_keep3"])
def test_holdout_split_marks_the_same_cells_without_a_session(problem, rule):
    X, (n_out, thresh, min_keep) = problem[0], rule
    want = reference(problem, rule)
    train, test = api.holdout_split(X, None if n_out == MAX else n_out, FRAC[thresh], min_keep, SEED)
    same_csr(test, want, np.float64)
    assert (train + test != X).nnz == 0 and train.nnz + test.nnz == X.nnz
    some = [15, 3, 11]
    test = api.holdout_split(X, None if n_out == MAX else n_out, FRAC[thresh], min_keep, SEED, users=some, use_float=True)[1]
    same_csr(test[some], reference(problem, rule, some), np.float32)
    assert test.nnz == test[some].nnz


def test_exclude_seen_forgets_the_held_out_cells_at_once(problem):
    X, u, rule = problem[0], 7, RULES[0]
    held = int(reference(problem, rule, [u]).indices[0])
    A, B = np.ones((X.shape[0], 4), np.float32), np.full((DIMB, 4), 0.25, np.float32)
    B[held] = 8.0
    s = session(X, True)
    s.set_factors(A, B)
    assert held not in s.topn_batch([u], 3, exclude_seen=True)[0][0]
    assert holdout(s, rule, users=[u]).nnz == 1
    assert s.topn_batch([u], 3, exclude_seen=True)[0][0][0] == held
    s.close()
