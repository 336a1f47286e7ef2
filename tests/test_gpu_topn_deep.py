"""Deep batched top-N (include/poismf_hip.h section 1l) on the GPU: items and score bits against the existing predict path at every
depth, with prunes forced and avoided, all ties, exclusions from the top of the list, short and empty rows, n_top above the number of
items, independence of the batch a user is in, agreement with the shallow call, the single-slice path and the host-pointer entry.

The expectation is built as in tests/test_gpu_topn_batch.py from Session.predict -- the pair_dot_kernel path, which the batched code
does not share: the user's whole score row, minus E(u), ordered by (score descending, item ascending) with np.lexsort, padded with
TOPN_NONE and -inf.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests import helpers as H

pytestmark = pytest.mark.gpu

DIMA, DIMB = 130, 3077            # two full tiles of users and one of two; 49 tiles of items
DEPTHS = (1, 10, 128, 129, 255, 256, 257, 1000, 1024)
ZERO_USER, FEW_USER, NONE_USER = 5, 7, 9   # a row of A that is zero; all but 5 items excluded; everything excluded


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def _factors(dimA, dimB, k, prec, seed):
    rng = np.random.default_rng(seed)
    dt = H.dtype_of(prec)
    return rng.random((dimA, k)).astype(dt), rng.random((dimB, k)).astype(dt)


def _score_rows(s, users, dimB):
    """the users' whole score rows from the existing predict path: [len(users) x dimB]"""
    users = np.asarray(users, np.uint64)
    out = s.predict(np.repeat(users, dimB), np.tile(np.arange(dimB, dtype=np.uint64), len(users)))
    return out.reshape(len(users), dimB)


def _expect(score_rows, excl, n):
    """[m x n] items and scores: every row's first n admissible items under (score descending, item ascending), then the padding"""
    m, dimB = score_rows.shape
    ix = np.full((m, n), api.TOPN_NONE, np.uint64)
    sc = np.full((m, n), -np.inf, score_rows.dtype)
    for i in range(m):
        idx = np.setdiff1d(np.arange(dimB), np.asarray(excl[i], np.int64))
        s = score_rows[i, idx]
        o = np.lexsort((idx, -s.astype(np.float64)))[:n]   # (the cast is exact; it only keeps -s in one dtype)
        ix[i, :len(o)] = idx[o]
        sc[i, :len(o)] = s[o]
    return ix, sc


def _excl_pair(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


def _same(got, want, n, what):
    """got [m x n] against the first n columns of want [m x >= n] (a row's padding starts where its admissible items end, at every n)"""
    ok_ix, ok_sc = np.array_equal(got[0], want[0][:, :n]), np.array_equal(got[1], want[1][:, :n])
    print(f"{what} n {n}: equal ix {ok_ix} equal score bits {ok_sc}")
    assert got[0].shape == (want[0].shape[0], n) and got[1].shape == got[0].shape
    if not ok_ix:
        bad = np.nonzero((got[0] != want[0][:, :n]).any(axis=1))[0]
        raise AssertionError((what, n, "rows", bad[:8].tolist(), got[0][bad[0]][:12], want[0][bad[0]][:12]))
    assert got[1].tobytes() == np.ascontiguousarray(want[1][:, :n]).tobytes(), (what, n)


def _near_the_top(A, B, step, depth):
    """per user, every step-th of its best `depth` items by a host product (which items they are exactly does not matter): sorted lists"""
    approx = A.astype(np.float64) @ B.astype(np.float64).T
    best = np.argsort(-approx, axis=1, kind="stable")[:, :depth:step]
    return [np.sort(r) for r in best]


def _session(dimA, dimB, k, prec, A, B, seen_rows=None):
    if seen_rows is None:
        seen_rows = [np.array([i % dimB]) for i in range(dimA)]
    row = np.concatenate([np.full(len(r), i) for i, r in enumerate(seen_rows)])
    col = np.concatenate(seen_rows)
    s = api.Session.from_coo(sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(dimA, dimB)), k, prec)
    s.set_factors(A, B)
    return s


KS = (3, 50, 65, 100)   # 65: two LDS chunks in fp32


@pytest.mark.parametrize("k", KS)
def test_bits_against_the_predict_path(prec, k):
    """every depth x {no exclusion, a batch list, exclude_seen, both}; the excluded items come from the top of the user's list, one user
    keeps 5 items, one keeps none, one row of A is zero (all ties: the smallest admissible indices with score 0)"""
    A, B = _factors(DIMA, DIMB, k, prec, 100 + k)
    A[ZERO_USER] = 0
    rng = np.random.default_rng(k)
    seen = _near_the_top(A, B, 2, 600)
    extra = _near_the_top(A, B, 3, 1024)
    everything = np.arange(DIMB)
    seen[FEW_USER + 4] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))   # (exclude_seen alone has its short rows too)
    seen[NONE_USER + 4] = everything
    extra[FEW_USER] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))
    extra[NONE_USER] = everything
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, users, DIMB)
        assert not rows[ZERO_USER].any()
        none = [np.empty(0, np.int64)] * DIMA
        both = [np.union1d(a, b) for a, b in zip(seen, extra)]
        want = {w: _expect(rows, e, max(DEPTHS)) for w, e in (("plain", none), ("list", extra), ("seen", seen), ("both", both))}
        assert want["plain"][0][ZERO_USER].tolist() == list(range(max(DEPTHS)))
        assert (want["list"][0][FEW_USER] != api.TOPN_NONE).sum() == 5 and (want["list"][0][NONE_USER] == api.TOPN_NONE).all()
        pair = _excl_pair(extra)
        for n in DEPTHS:
            _same(s.topn_deep(users, n, output_score=True), want["plain"], n, "plain")
            _same(s.topn_deep(users, n, exclude=pair, output_score=True), want["list"], n, "list")
            _same(s.topn_deep(users, n, exclude_seen=True, output_score=True), want["seen"], n, "seen")
            _same(s.topn_deep(users, n, exclude_seen=True, exclude=pair, output_score=True), want["both"], n, "both")
        ix, sc = s.topn_deep(users, 1000)
        assert np.array_equal(ix, want["plain"][0][:, :1000]) and sc.size == 0
    finally:
        s.close()


@pytest.mark.parametrize("direction", ["rising", "falling"])
def test_worst_and_best_case_for_the_lists(prec, direction):
    """B's rows are one base vector times a factor that rises with the item index (every item beats the threshold: the most appends
    and prunes) or falls (no append after the first n_top); 8192 users leave 4 slices of 3000 items, longer than every list"""
    dimA, dimB, k = 8192, 12000, 8
    rng = np.random.default_rng(12)
    dt = H.dtype_of(prec)
    A = (0.5 + rng.random((dimA, k))).astype(dt)
    A[ZERO_USER] = 0
    f = 1.0 + np.arange(dimB) / dimB
    B = (np.outer(f if direction == "rising" else f[::-1], 0.5 + rng.random(k))).astype(dt)
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        users = np.arange(dimA, dtype=np.uint64)
        sample = np.concatenate([[0, ZERO_USER, 63, 64, dimA - 1], rng.choice(dimA, 27, replace=False)])
        rows = _score_rows(s, sample, dimB)
        assert direction == "falling" or np.all(np.diff(rows[0]) >= 0)
        want = _expect(rows, [np.empty(0, np.int64)] * len(sample), 1024)
        for n in (1, 129, 1000, 1024):
            ix, sc = s.topn_deep(users, n, output_score=True)
            _same((ix[sample], sc[sample]), want, n, direction)
    finally:
        s.close()


def test_prunes_in_the_walk_on_random_scores(prec):
    """8192 users leave 4 slices of 3000 items: lists of 2048 entries fill and are pruned several times at n_top = 1000"""
    dimA, dimB, k = 8192, 12000, 8
    A, B = _factors(dimA, dimB, k, prec, 21)
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        rng = np.random.default_rng(4)
        users = np.arange(dimA, dtype=np.uint64)
        sample = np.sort(rng.choice(dimA, 32, replace=False))
        seen = [np.array([u % dimB]) for u in sample]
        want = _expect(_score_rows(s, sample, dimB), seen, 1000)
        for n in (300, 1000):
            ix, sc = s.topn_deep(users, n, exclude_seen=True, output_score=True)
            _same((ix[sample], sc[sample]), want, n, "prunes")
    finally:
        s.close()


def test_n_top_above_the_number_of_items(prec):
    dimA, dimB, k = 70, 300, 4
    A, B = _factors(dimA, dimB, k, prec, 3)
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        users = np.arange(dimA, dtype=np.uint64)
        want = _expect(_score_rows(s, users, dimB), [np.empty(0, np.int64)] * dimA, 1024)
        got = s.topn_deep(users, 1024, output_score=True)
        _same(got, want, 1024, "above-dimB")
        assert np.all(got[0][:, 300:] == api.TOPN_NONE) and np.all(got[1][:, 300:] == -np.inf) and np.all(got[0][:, :300] < 300)
    finally:
        s.close()


def test_independence_of_company(prec):
    """the same user three times in a batch and alone; batches of 1, 63, 64 and 65 users: equal rows, bit for bit"""
    k, n = 50, 257
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        ix_all, sc_all = s.topn_deep(everyone, n, exclude_seen=True, output_score=True)
        ix_rev, sc_rev = s.topn_deep(everyone[::-1].copy(), n, exclude_seen=True, output_score=True)
        assert np.array_equal(ix_rev[::-1], ix_all) and sc_rev[::-1].tobytes() == sc_all.tobytes()
        for u in (0, 63, 64, 129):
            ix3, sc3 = s.topn_deep([u, 11, u, 100, u], n, exclude_seen=True, output_score=True)
            for p in (0, 2, 4):
                assert np.array_equal(ix3[p], ix_all[u]) and sc3[p].tobytes() == sc_all[u].tobytes()
            assert np.array_equal(ix3[1], ix_all[11]) and np.array_equal(ix3[3], ix_all[100])
        for m in (1, 63, 64, 65):
            ix, sc = s.topn_deep(everyone[40:40 + m], n, exclude_seen=True, output_score=True)
            assert np.array_equal(ix, ix_all[40:40 + m]) and sc.tobytes() == sc_all[40:40 + m].tobytes()
        again = s.topn_deep(everyone, n, exclude_seen=True, output_score=True)
        assert again[0].tobytes() == ix_all.tobytes() and again[1].tobytes() == sc_all.tobytes()
    finally:
        s.close()


def test_agreement_with_the_shallow_call(prec):
    """n_top of 10 and 128: Session.topn_batch's items and score bits, on one session (they share its scratch, in either order)"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 8)
    seen = _near_the_top(A, B, 2, 300)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        pair = _excl_pair(_near_the_top(A, B, 3, 300))
        for n in (10, 128):
            shallow = s.topn_batch(users, n, exclude_seen=True, exclude=pair, output_score=True)
            deep = s.topn_deep(users, n, exclude_seen=True, exclude=pair, output_score=True)
            assert np.array_equal(deep[0], shallow[0]) and deep[1].tobytes() == shallow[1].tobytes()
        deep = s.topn_deep(users, 1024, output_score=True)          # grows the shared scratch ...
        shallow = s.topn_batch(users, 128, output_score=True)       # ... under the shallow call
        assert np.array_equal(deep[0][:, :128], shallow[0]) and np.ascontiguousarray(deep[1][:, :128]).tobytes() == shallow[1].tobytes()
    finally:
        s.close()


def test_single_slice_path(prec):
    """enough users that the items are not sliced: the tile kernel's lists are the result (no merge)"""
    dimA, dimB, k, n = 49152, 300, 4, 200
    A, B = _factors(dimA, dimB, k, prec, 14)
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        ix, sc = s.topn_deep(np.arange(dimA, dtype=np.uint64), n, exclude_seen=True, output_score=True)
        rng = np.random.default_rng(2)
        sample = np.sort(np.concatenate([[0, 63, 64, dimA - 1], rng.choice(dimA, 252, replace=False)]))
        want = _expect(_score_rows(s, sample, dimB), [np.array([u % dimB]) for u in sample], n)   # (predict for the sampled rows only)
        _same((ix[sample], sc[sample]), want, n, "single-slice")
        # n_top = 1: lists of 128 entries over 300 items -- this path's prunes
        ix1, sc1 = s.topn_deep(np.arange(dimA, dtype=np.uint64), 1, exclude_seen=True, output_score=True)
        _same((ix1[sample], sc1[sample]), want, 1, "single-slice-n1")
    finally:
        s.close()


def test_host_pointer_entry_and_model(prec):
    """poismf_hip_topn_deep / PoisMF.topN_deep: the session call's rows, bit for bit"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 41)
    seen = _near_the_top(A, B, 2, 600)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        users = np.array([3, 129, 64, 3, 77, 0], np.uint64)
        pair = _excl_pair([seen[u] for u in users])
        for n in (129, 1000):
            a = s.topn_deep(users, n, exclude_seen=True, output_score=True)
            b = m.topN_deep(users, n, exclude=pair, output_score=True)            # (the batch's rows of A only)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        everyone = np.arange(DIMA)
        a = s.topn_deep(everyone, 1000, output_score=True)
        b = m.topN_deep(everyone, output_score=True)                              # (all of A goes up; n = 1000 is the default)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        c = m.topN_deep(everyone)
        assert np.array_equal(c[0], a[0]) and c[1].size == 0
    finally:
        s.close()
