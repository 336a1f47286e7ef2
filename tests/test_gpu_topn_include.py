"""Batched top-N over per-user include lists (include/poismf_hip.h section 1h) on the GPU: bits against the existing predict path,
equivalence with the dense batched kernel on the complement, padding of short rows, ties, independence of the batch a user is in,
chunking, the host-pointer entry and PoisMF.topN_batch, the cross-check with the single-user topN, and the argument checks on a
machine that has a device.

The expectation of the exact tests is built from Session.predict -- the pair_dot_kernel path, which the new kernel does not share:
the user's scores restricted to I(u) \\ E(u), ordered by (score descending, item ascending) with np.lexsort, padded with TOPN_NONE /
-inf.  np.array_equal on indices and scores: no tolerance and no user left out (only tests.helpers.check_topn has one)."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.test_topn_include_cpu import BAD, FULL, _c_include

pytestmark = pytest.mark.gpu

MERGE_MAX = 2048
DIMA = 300


def T(is_float, t64, t32):
    return t32 if is_float else t64


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def _slice(length, n):
    return int(api.load_library(True).poismf_hip_topn_include_slice(int(length), int(n)))


class _World:
    """sizes from the slice aid, one user per list length, and a matrix of seen items -- built once and never changed"""

    def __init__(self):
        S = self.S = _slice(0, 128)
        grow = (MERGE_MAX // 128) * S
        while True:   # the smallest length at which a slice at n_top = 128 grows past the minimum
            if _slice(grow, 128) > S:
                break
            grow += 1
        assert _slice(grow - 1, 128) == S
        self.grow = grow
        self.dimB = grow + 999          # a full-catalogue list at n_top = 128 needs slices longer than the minimum
        assert _slice(self.dimB, 128) > S
        lengths = sorted(set(range(0, 201)) | {S - 1, S, S + 1, 2 * S + 1, self.dimB, grow - 1, grow, grow + 1})
        assert len(lengths) <= DIMA
        rng = np.random.default_rng(12)
        self.users = rng.choice(DIMA, len(lengths), replace=False).astype(np.uint64)
        self.lists = [np.arange(self.dimB) if ln == self.dimB else np.sort(rng.choice(self.dimB, ln, replace=False)) for ln in lengths]
        # seen items: ~60 per user anywhere, half of every list up to 40 candidates, and the whole list for lengths 1..5 and 150
        row, col = [rng.integers(0, DIMA, 60 * DIMA)], [rng.integers(0, self.dimB, 60 * DIMA)]
        for u, lst in zip(self.users, self.lists):
            take = lst if len(lst) in (1, 2, 3, 4, 5, 150) else lst[::2] if len(lst) <= 40 else lst[:0]
            row.append(np.full(len(take), int(u)))
            col.append(take)
        row, col = np.concatenate(row), np.concatenate(col)
        self.coo = sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(DIMA, self.dimB))
        csr = sp.csr_matrix(self.coo)
        csr.sum_duplicates(); csr.sort_indices()
        self.seen = [csr.indices[csr.indptr[u]:csr.indptr[u + 1]].astype(np.int64) for u in self.users.astype(np.int64)]
        self.extra = [np.sort(rng.choice(self.dimB, int(rng.integers(0, 300)), replace=False)) for _ in self.users]
        self.none = [np.empty(0, np.int64)] * len(self.users)
        self.both = [np.union1d(a, b) for a, b in zip(self.seen, self.extra)]
        self.incl = _pair(self.lists)


def _pair(rows):
    """(indptr, indices) of per-user sorted lists"""
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


@pytest.fixture(scope="module")
def world():
    return _World()


def _factors(dimA, dimB, k, prec, seed):
    rng = np.random.default_rng(seed)
    dt = H.dtype_of(prec)
    return rng.random((dimA, k)).astype(dt), rng.random((dimB, k)).astype(dt)


def _session(coo, k, prec, A, B):
    s = api.Session.from_coo(coo, k, prec)
    s.set_factors(A, B)
    return s


def _cell_scores(s, users, lists):
    """the scores of every (user, candidate) cell from the existing predict path, one array per user"""
    u = np.repeat(np.asarray(users, np.uint64), [len(l) for l in lists])
    j = np.concatenate(lists).astype(np.uint64) if len(lists) else np.empty(0, np.uint64)
    out = s.predict(u, j) if len(u) else np.empty(0)
    return np.split(out, np.cumsum([len(l) for l in lists])[:-1])


def _expect(lst, scores, excluded, n):
    """the first n of lst minus excluded under (score descending, item ascending), padded; and how many are real"""
    keep = ~np.isin(lst, excluded)
    idx, sc = np.asarray(lst, np.int64)[keep], scores[keep]
    o = np.lexsort((idx, -sc.astype(np.float64)))[:n]   # (the cast is exact; it only keeps -sc in one dtype)
    eix = np.full(n, api.TOPN_NONE, np.uint64)
    esc = np.full(n, -np.inf, scores.dtype)
    eix[:len(o)], esc[:len(o)] = idx[o].astype(np.uint64), sc[o]
    return eix, esc, len(o)


def _assert_rows(got, users, lists, scores, excl, n, what):
    ix, sc = got
    assert ix.shape == (len(users), n) and sc.shape == (len(users), n)
    bad = []
    for i in range(len(users)):
        eix, esc, real = _expect(lists[i], scores[i], excl[i], n)
        if not (np.array_equal(ix[i], eix) and np.array_equal(sc[i], esc)):
            bad.append((what, int(users[i]), len(lists[i]), n, real))
        assert int(np.sum(ix[i] != api.TOPN_NONE)) == real == min(n, len(np.setdiff1d(lists[i], excl[i])))
    print(f"{what} n {n}: {len(users) - len(bad)} of {len(users)} rows equal")
    assert not bad, bad[:10]


KS = [1, 3, 4, 5, 50, 64, 65, 100, 200, 256]
BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_bits_against_the_predict_path(world, prec, k):
    """1. and 3. indices and scores array_equal to the lexsort of Session.predict's scores over I(u) minus E(u), padding included"""
    w = world
    A, B = _factors(DIMA, w.dimB, k, prec, 10 + k)
    s = _session(w.coo, k, prec, A, B)
    try:
        scores = _cell_scores(s, w.users, w.lists)
        for n in (1, 10, 128):
            _assert_rows(s.topn_batch(w.users, n, include=w.incl, output_score=True), w.users, w.lists, scores, w.none, n, "plain")
            _assert_rows(s.topn_batch(w.users, n, include=w.incl, exclude_seen=True, output_score=True), w.users, w.lists, scores, w.seen, n, "seen")
            _assert_rows(s.topn_batch(w.users, n, include=w.incl, exclude=_pair(w.extra), output_score=True), w.users, w.lists, scores, w.extra, n,
                         "extra")
            _assert_rows(s.topn_batch(w.users, n, include=w.incl, exclude_seen=True, exclude=_pair(w.extra), output_score=True), w.users, w.lists,
                         scores, w.both, n, "both")
    finally:
        s.close()


def test_equivalence_with_the_dense_kernel(world, prec):
    """2. where |I \\ E| >= n the rows equal the dense batched top-N's for the exclusion set E united with the complement of I"""
    w, k = world, 50
    A, B = _factors(DIMA, w.dimB, k, prec, 21)
    s = _session(w.coo, k, prec, A, B)
    try:
        everything = np.arange(w.dimB)
        for n in (10, 128):
            pick = [i for i in range(len(w.users)) if len(np.setdiff1d(w.lists[i], w.both[i])) >= n]
            assert len(pick) > 20
            users = w.users[pick]
            lists, extra = [w.lists[i] for i in pick], [w.extra[i] for i in pick]
            a = s.topn_batch(users, n, include=_pair(lists), exclude_seen=True, exclude=_pair(extra), output_score=True)
            dense = [np.union1d(np.setdiff1d(everything, l), e) for l, e in zip(lists, extra)]
            b = s.topn_batch(users, n, exclude_seen=True, exclude=_pair(dense), output_score=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        s.close()


def test_padding(world, prec):
    """3. short lists, lists emptied by exclude_seen, an empty list: TOPN_NONE / -inf after the |I \\ E| real entries"""
    w, k = world, 7
    A, B = _factors(DIMA, w.dimB, k, prec, 33)
    s = _session(w.coo, k, prec, A, B)
    try:
        ix, sc = s.topn_batch(w.users, 128, include=w.incl, exclude_seen=True, output_score=True)
        emptied = 0
        for i, lst in enumerate(w.lists):
            real = len(np.setdiff1d(lst, w.seen[i]))
            emptied += len(lst) > 0 and real == 0
            c = min(real, 128)
            assert np.all(ix[i, :c] != api.TOPN_NONE) and np.all(np.isfinite(sc[i, :c]))
            assert np.all(ix[i, c:] == api.TOPN_NONE) and np.all(sc[i, c:] == -np.inf)
            assert np.isin(ix[i, :c].astype(np.int64), lst).all() and not np.isin(ix[i, :c].astype(np.int64), w.seen[i]).any()
        assert emptied >= 5 and len(w.lists[0]) == 0
        # every list empty, and no index array at all
        ix, sc = s.topn_batch(w.users[:5], 10, include=(np.zeros(6, np.uint64), np.empty(0, np.uint64)), output_score=True)
        assert np.all(ix == api.TOPN_NONE) and np.all(sc == -np.inf)
        ix, _ = s.topn_batch(w.users[:5], 10, include=sp.csr_matrix((5, w.dimB)))
        assert np.all(ix == api.TOPN_NONE)
    finally:
        s.close()


def test_ties(world, prec):
    """4. blocks of identical rows of B: item index ascending; an all-zero A[u]: the first n indices of the list"""
    w, k = world, 50
    A, B = _factors(DIMA, w.dimB, k, prec, 5)
    rng = np.random.default_rng(9)
    B[:200] *= 1.5                          # (so that the duplicated rows are among the best: ties at the top)
    dst = w.dimB - 1 - rng.choice(w.dimB // 2, 200, replace=False)
    B[dst] = B[:200]
    B[dst[:50] - w.dimB // 4] = B[:50]       # some scores three times
    B[3000:3100] = B[3000]                  # a block of a hundred equal rows
    zero = int(w.users[-1])
    A[zero] = 0
    s = _session(w.coo, k, prec, A, B)
    try:
        scores = _cell_scores(s, w.users, w.lists)
        for n in (1, 10, 128):
            first = s.topn_batch(w.users, n, include=w.incl, output_score=True)
            _assert_rows(first, w.users, w.lists, scores, w.none, n, "ties")
            again = s.topn_batch(w.users, n, include=w.incl, output_score=True)
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
            lst = w.lists[-1]
            c = min(n, len(lst))
            assert np.array_equal(first[0][-1, :c], lst[:c].astype(np.uint64)) and np.all(first[1][-1, :c] == 0)
        long_ = [np.arange(w.dimB)] * 3     # the tied blocks whole, across slices
        sc3 = _cell_scores(s, w.users[:3], long_)
        _assert_rows(s.topn_batch(w.users[:3], 128, include=_pair(long_), output_score=True), w.users[:3], long_, sc3, w.none[:3], 128, "ties-long")
    finally:
        s.close()


def test_independence_of_company(world, prec):
    """5. the same (user, list): alone, among all users, in a reversed batch, and three times in one batch with three lists"""
    w, k = world, 50
    A, B = _factors(DIMA, w.dimB, k, prec, 77)
    s = _session(w.coo, k, prec, A, B)
    try:
        ix_all, sc_all = s.topn_batch(w.users, 10, include=w.incl, exclude_seen=True, output_score=True)
        ix_rev, sc_rev = s.topn_batch(w.users[::-1].copy(), 10, include=_pair(w.lists[::-1]), exclude_seen=True, output_score=True)
        assert np.array_equal(ix_rev[::-1], ix_all) and np.array_equal(sc_rev[::-1], sc_all)
        n_u = len(w.users)
        for i in (0, 1, 9, 64, 65, 130, 200, n_u - 6, n_u - 3, n_u - 2, n_u - 1):
            ix1, sc1 = s.topn_batch(w.users[i:i + 1], 10, include=_pair(w.lists[i:i + 1]), exclude_seen=True, output_score=True)
            assert np.array_equal(ix1[0], ix_all[i]) and np.array_equal(sc1[0], sc_all[i])
            # user i three times, with its own list, list 150's and the full catalogue; between them another user
            u, other = w.users[i], w.users[77]
            batch = np.array([u, other, u, u], np.uint64)
            lists = [w.lists[i], w.lists[77], w.lists[150], w.lists[-1]]
            ix3, sc3 = s.topn_batch(batch, 10, include=_pair(lists), exclude_seen=True, output_score=True)
            assert np.array_equal(ix3[0], ix_all[i]) and np.array_equal(sc3[0], sc_all[i])
            assert np.array_equal(ix3[1], ix_all[77]) and np.array_equal(sc3[1], sc_all[77])
            for p, l in ((2, 150), (3, n_u - 1)):
                ixa, sca = s.topn_batch([u], 10, include=_pair([w.lists[l]]), exclude_seen=True, output_score=True)
                assert np.array_equal(ix3[p], ixa[0]) and np.array_equal(sc3[p], sca[0])
    finally:
        s.close()


def test_chunking():
    """6. 3000 users x 25000 candidates: more indices than one chunk's index area holds; rows equal those of 64 users at a time"""
    dimA, dimB, k, n = 3000, 25000, 8, 10
    rng = np.random.default_rng(4)
    coo = sp.coo_matrix((np.ones(30 * dimA), (rng.integers(0, dimA, 30 * dimA), rng.integers(0, dimB, 30 * dimA))), shape=(dimA, dimB))
    A, B = _factors(dimA, dimB, k, True, 8)
    s = _session(coo, k, True, A, B)
    try:
        users = np.arange(dimA, dtype=np.uint64)
        n_cells = dimA * dimB
        assert n_cells > api.TOPN_INCLUDE_MAX_ROW, "the batch does not exceed one chunk's index area"
        assert 4 * n_cells > int(s.lib.poismf_hip_topn_include_scratch_bytes(dimA, n_cells, n, dimB, k)), "the lists fit the scratch whole"

        def full(m):
            return np.arange(m + 1, dtype=np.uint64) * np.uint64(dimB), np.tile(np.arange(dimB, dtype=np.uint64), m)

        ix, sc = s.topn_batch(users, n, include=full(dimA), exclude_seen=True, output_score=True)
        inc64 = full(64)
        for u0 in range(0, dimA, 64):
            m = min(64, dimA - u0)
            ix1, sc1 = s.topn_batch(users[u0:u0 + m], n, include=inc64 if m == 64 else full(m), exclude_seen=True, output_score=True)
            assert np.array_equal(ix1, ix[u0:u0 + m]) and np.array_equal(sc1, sc[u0:u0 + m]), u0
        csr = sp.csr_matrix(coo)
        csr.sum_duplicates(); csr.sort_indices()
        sample = np.sort(rng.choice(dimA, 32, replace=False)).astype(np.uint64)
        lists = [np.arange(dimB)] * 32
        scores = _cell_scores(s, sample, lists)
        seen = [csr.indices[csr.indptr[u]:csr.indptr[u + 1]] for u in sample.astype(np.int64)]
        _assert_rows((ix[sample.astype(np.int64)], sc[sample.astype(np.int64)]), sample, lists, scores, seen, n, "chunks")
    finally:
        s.close()


def test_host_pointer_entry_and_model(world, prec):
    """7. poismf_hip_topn_include / PoisMF.topN_batch(include=...): the session call's rows, bit for bit; the scratch is reused"""
    w, k = world, 50
    A, B = _factors(DIMA, w.dimB, k, prec, 41)
    s = _session(w.coo, k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, w.dimB, True
    try:
        for n in (10, 128):
            a = s.topn_batch(w.users, n, include=w.incl, exclude_seen=True, output_score=True)
            a2 = s.topn_batch(w.users, n, include=w.incl, exclude_seen=True, output_score=True)   # (same scratch, second call)
            assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
            b = m.topN_batch(w.users, n, exclude=_pair(w.seen), include=w.incl, output_score=True)     # (the batch's rows of A only)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        everyone = np.arange(DIMA, dtype=np.uint64)
        rng = np.random.default_rng(2)
        lists = [np.sort(rng.choice(w.dimB, 300, replace=False)) for _ in everyone]
        X = sp.csr_matrix((np.ones(300 * DIMA), np.concatenate(lists), np.arange(DIMA + 1) * 300), shape=(DIMA, w.dimB))
        a = s.topn_batch(everyone, 10, include=X, output_score=True)
        b = m.topN_batch(everyone, 10, include=X, output_score=True)                                   # (all of A goes up)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = m.topN_batch(everyone, 10, include=_pair(lists))
        assert np.array_equal(c[0], a[0]) and c[1].size == 0
        d = s.topn_batch(everyone, 10, output_score=True)   # the dense call after it, in the same scratch
        assert d[0].shape == (DIMA, 10) and np.all(d[1][:, 0] >= a[1][:, 0])
    finally:
        s.close()


def test_cross_check_with_the_single_user_topn(world, prec):
    """8. Session.topn(u, n, include_ix=list) and the new row both pass check_topn; they may differ only where it allows"""
    w, k, n = world, 50, 10
    A, B = _factors(DIMA, w.dimB, k, prec, 31)
    s = _session(w.coo, k, prec, A, B)
    none = np.empty(0, np.uint64)
    rtol = T(prec, 1e-13, 1e-5)
    try:
        pick = [i for i in range(len(w.users)) if len(w.lists[i]) >= 40][::11][:16]
        assert len(pick) == 16
        ix, sc = s.topn_batch(w.users[pick], n, include=_pair([w.lists[i] for i in pick]), output_score=True)
        for r, i in enumerate(pick):
            u, lst = int(w.users[i]), w.lists[i].astype(np.uint64)
            ix1, sc1 = s.topn(u, n, include_ix=lst, output_score=True)
            H.check_topn(A[u], B, ix1, sc1, lst, none, n, rtol)
            H.check_topn(A[u], B, ix[r], sc[r], lst, none, n, rtol)
    finally:
        s.close()


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_errors_with_a_device(flavour, case):
    """9. rc 2 and nothing written, through the C entry point itself"""
    users, n, incl, excl = BAD[case]
    rc, out, sc = _c_include(flavour, users, n, incl, excl)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_valid_call_with_a_device(flavour):
    rc, out, sc = _c_include(flavour, [0, 1, 0], 4, ([0, 3, 3, 9], [7, 8, 9, 0, 1, 2, 3, 4, 5]), ([0, 1, 1, 3], [8, 0, 4]))
    assert rc == 0
    none = -1 if flavour == "r" else api.TOPN_NONE
    # all scores are equal (factors of ones): ascending item indices, the user's exclusions left out, short rows padded
    assert out.tolist() == [[7, 9, none, none], [none] * 4, [1, 2, 3, 5]]
    assert sc.tolist() == [[3.0, 3.0, -np.inf, -np.inf], [-np.inf] * 4, [3.0] * 4]


def test_session_errors_with_a_device(prec):
    """9. the session entry: exclude_seen for a user outside the shard, a NULL include list: rc 2, nothing written"""
    k, dimB = 8, 2000
    rng = np.random.default_rng(3)
    coo = sp.coo_matrix((np.ones(6000), (rng.integers(0, DIMA, 6000), rng.integers(0, dimB, 6000))), shape=(DIMA, dimB))
    csr, csc = harness.process_data(coo, prec)
    A, B = _factors(DIMA, dimB, k, prec, 3)
    s = api.Session(csr, csc, DIMA, dimB, k, prec, shardA=(100, 200), shardB=(0, dimB))
    try:
        s.set_factors(A, B)
        users = np.array([150, 200], np.uint64)
        ip, ii = np.array([0, 2, 4], np.uint64), np.array([5, 9, 1, 7], np.uint64)
        out = np.full((2, 5), 12345, np.uint64)
        p = api._ptr
        assert s.lib.poismf_hip_session_topn_include(s.h, p(users), 2, 5, p(ip), p(ii), 1, None, None, p(out), None) == 2
        assert s.lib.poismf_hip_session_topn_include(s.h, p(users), 2, 5, None, None, 0, None, None, p(out), None) == 2
        assert np.all(out == 12345)
        with pytest.raises(ValueError):
            s.topn_batch(users, 5, exclude_seen=True, include=(ip, ii))
        ix, _ = s.topn_batch(users, 5, include=(ip, ii))     # without exclude_seen any user of A may be asked for
        assert sorted(ix[0, :2].tolist()) == [5, 9] and np.all(ix[:, 2:] == api.TOPN_NONE)
        ix, _ = s.topn_batch([100, 199], 5, exclude_seen=True, include=(ip, ii))
        assert ix.shape == (2, 5)
    finally:
        s.close()
