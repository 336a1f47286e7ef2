"""Batched top-N over candidate lists shared between users (include/poismf_hip.h section 1i) on the GPU: bits against the existing
predict path, equality with the per-user include lists of section 1h and with the dense kernel on the complement, padding of short
rows, ties and phantom rows, independence of the company a user is in, slices, chunking, the host-pointer entry and
PoisMF.topN_batch, and the argument checks on a machine that has a device.

The expectation of the exact tests is built from Session.predict -- the pair_dot_kernel path, which the new kernel does not share:
the user's scores restricted to L \\ E(u), ordered by (score descending, item ascending) with np.lexsort, padded with TOPN_NONE /
-inf.  np.array_equal on indices and scores: no tolerance and no user left out."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.test_topn_shared_cpu import BAD, _c_shared

pytestmark = pytest.mark.gpu

DIMA, DIMB = 400, 4099
# list length -> users that refer to it; the list of 77 items is in the table and has no user
GROUPS = {0: 3, 1: 2, 9: 1, 10: 5, 11: 4, 63: 63, 64: 64, 65: 65, 127: 6, 128: 7, 129: 130, 1000: 20, DIMB: 20, 77: 0}
HALVED, EMPTIED = (10, 64, 1000), (9,)      # lists that lose every other item / all items to the users' seen items


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def _pair(rows):
    """(indptr, indices) of sorted lists"""
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


class _World:
    """the table of lists, an interleaved batch with repeated users, and a matrix of seen items -- built once and never changed"""

    def __init__(self):
        rng = np.random.default_rng(12)
        assert DIMB % 64 != 0
        self.lengths = list(GROUPS)
        self.table = [np.arange(DIMB) if ln == DIMB else np.sort(rng.choice(DIMB, ln, replace=False)) for ln in self.lengths]
        assert self.table[self.lengths.index(DIMB)][-1] == DIMB - 1
        self.G = len(self.table)
        self.incl = _pair(self.table)
        of = np.concatenate([np.full(c, g) for g, c in enumerate(GROUPS.values())])
        assert len(of) == 390 and {0, 1, 63, 64, 65, 130} <= set(GROUPS.values())
        users = rng.choice(DIMA, len(of), replace=False)
        # repeats: users of the 129-list again on the same list, on the 1000-list and on the full catalogue
        again = users[of == self.lengths.index(129)][:9]
        users = np.concatenate([users, again])
        of = np.concatenate([of, np.repeat([self.lengths.index(129), self.lengths.index(1000), self.lengths.index(DIMB)], 3)])
        order = rng.permutation(len(of))             # the groups interleaved
        self.users, self.of = users[order].astype(np.uint64), of[order].astype(np.int64)
        assert not np.all(np.diff(self.of) >= 0) and len(np.unique(self.users)) < len(self.users)
        self.lists = [self.table[g] for g in self.of]      # every batch entry's list written out (what section 1h takes)
        # seen items: ~30 per user anywhere; every other item of some lists; the whole of a short list
        row, col = [rng.integers(0, DIMA, 30 * DIMA)], [rng.integers(0, DIMB, 30 * DIMA)]
        for u, g in zip(self.users, self.of):
            ln = self.lengths[g]
            take = self.table[g][::2] if ln in HALVED else self.table[g] if ln in EMPTIED else self.table[g][:0]
            row.append(np.full(len(take), int(u)))
            col.append(take)
        row, col = np.concatenate(row), np.concatenate(col)
        self.coo = sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(DIMA, DIMB))
        csr = sp.csr_matrix(self.coo)
        csr.sum_duplicates(); csr.sort_indices()
        self.seen = [csr.indices[csr.indptr[u]:csr.indptr[u + 1]].astype(np.int64) for u in self.users.astype(np.int64)]
        self.extra = [np.sort(rng.choice(DIMB, int(rng.integers(0, 200)), replace=False)) for _ in self.users]
        self.none = [np.empty(0, np.int64)] * len(self.users)
        self.both = [np.union1d(a, b) for a, b in zip(self.seen, self.extra)]


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
            bad.append((what, i, int(users[i]), len(lists[i]), n, real))
        assert int(np.sum(ix[i] != api.TOPN_NONE)) == real == min(n, len(np.setdiff1d(lists[i], excl[i])))
    print(f"{what} n {n}: {len(users) - len(bad)} of {len(users)} rows equal")
    assert not bad, bad[:10]


KS = [1, 3, 4, 5, 32, 33, 50, 64, 65, 100, 256]      # (TB_KC is 64 columns in fp32 and 32 in fp64)
BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_bits_against_the_predict_path(world, prec, k):
    """1. indices and scores array_equal to the lexsort of Session.predict's scores over L minus E(u), padding included"""
    w = world
    A, B = _factors(DIMA, DIMB, k, prec, 10 + k)
    s = _session(w.coo, k, prec, A, B)
    try:
        scores = _cell_scores(s, w.users, w.lists)
        kw = dict(include=w.incl, include_of=w.of, output_score=True)
        for n in (1, 10, 128):
            _assert_rows(s.topn_batch(w.users, n, **kw), w.users, w.lists, scores, w.none, n, "plain")
            _assert_rows(s.topn_batch(w.users, n, exclude_seen=True, **kw), w.users, w.lists, scores, w.seen, n, "seen")
            _assert_rows(s.topn_batch(w.users, n, exclude=_pair(w.extra), **kw), w.users, w.lists, scores, w.extra, n, "extra")
            _assert_rows(s.topn_batch(w.users, n, exclude_seen=True, exclude=_pair(w.extra), **kw), w.users, w.lists, scores, w.both, n, "both")
    finally:
        s.close()


def test_equality_with_the_include_lists_and_the_dense_kernel(world, prec):
    """2. the same batch with every user's list written out (section 1h): every row equal; and the dense call with the complement
    as `exclude` on the rows that have at least n admissible items"""
    w, k = world, 50
    A, B = _factors(DIMA, DIMB, k, prec, 21)
    s = _session(w.coo, k, prec, A, B)
    try:
        everything = np.arange(DIMB)
        written = _pair(w.lists)
        for n in (1, 10, 128):
            for kw in (dict(), dict(exclude_seen=True), dict(exclude_seen=True, exclude=_pair(w.extra))):
                a = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, output_score=True, **kw)
                b = s.topn_batch(w.users, n, include=written, output_score=True, **kw)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (n, kw.keys())
            pick = [i for i in range(len(w.users)) if len(np.setdiff1d(w.lists[i], w.both[i])) >= n]
            assert len(pick) > 20
            dense = [np.union1d(np.setdiff1d(everything, w.lists[i]), w.extra[i]) for i in pick]
            d = s.topn_batch(w.users[pick], n, exclude_seen=True, exclude=_pair(dense), output_score=True)
            assert np.array_equal(a[0][pick], d[0]) and np.array_equal(a[1][pick], d[1]), n
    finally:
        s.close()


def test_padding(world, prec):
    """3. n above the list's length, lists emptied by exclusion, the empty list: TOPN_NONE / -inf after the |L \\ E| real entries"""
    w, k = world, 7
    A, B = _factors(DIMA, DIMB, k, prec, 33)
    s = _session(w.coo, k, prec, A, B)
    try:
        ix, sc = s.topn_batch(w.users, 128, include=w.incl, include_of=w.of, exclude_seen=True, output_score=True)
        emptied = empty = short = 0
        for i, lst in enumerate(w.lists):
            real = len(np.setdiff1d(lst, w.seen[i]))
            emptied += len(lst) > 0 and real == 0
            empty += len(lst) == 0
            short += 0 < real < 128
            c = min(real, 128)
            assert np.all(ix[i, :c] != api.TOPN_NONE) and np.all(np.isfinite(sc[i, :c]))
            assert np.all(ix[i, c:] == api.TOPN_NONE) and np.all(sc[i, c:] == -np.inf)
            assert np.isin(ix[i, :c].astype(np.int64), lst).all() and not np.isin(ix[i, :c].astype(np.int64), w.seen[i]).any()
        assert emptied >= 1 and empty == 3 and short > 100
        # a table of empty lists, and no index array at all
        ix, sc = s.topn_batch(w.users[:5], 10, include=(np.zeros(3, np.uint64), np.empty(0, np.uint64)), include_of=[0, 1, 1, 0, 1], output_score=True)
        assert np.all(ix == api.TOPN_NONE) and np.all(sc == -np.inf)
        ix, _ = s.topn_batch(w.users[:5], 10, include=sp.csr_matrix((1, DIMB)), include_of=0)
        assert np.all(ix == api.TOPN_NONE)
    finally:
        s.close()


def test_ties_and_phantoms(world, prec):
    """4. blocks of identical rows of B come back in item order; an all-zero A[u] gets the first n admissible items of its list with
    score 0 and never a position past the list's end (lists of 65 and 129 items: one and one candidate into their last step)"""
    w, k = world, 50
    A, B = _factors(DIMA, DIMB, k, prec, 5)
    rng = np.random.default_rng(9)
    B[:200] *= 1.5                          # (so that the duplicated rows are among the best: ties at the top)
    dst = DIMB - 1 - rng.choice(DIMB // 2, 200, replace=False)
    B[dst] = B[:200]
    B[3000:3100] = B[3000]                  # a block of a hundred equal rows
    l65, l129 = w.lengths.index(65), w.lengths.index(129)
    for g in (l65, l129):                   # the lists' own items in tied pairs as well
        B[w.table[g][1::2]] = B[w.table[g][:len(w.table[g]) - 1:2]]
    zeros = [int(np.flatnonzero(w.of == g)[0]) for g in (l65, l129)]
    for i in zeros:
        A[int(w.users[i])] = 0
    s = _session(w.coo, k, prec, A, B)
    try:
        scores = _cell_scores(s, w.users, w.lists)
        for n in (1, 10, 128):
            first = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, output_score=True)
            _assert_rows(first, w.users, w.lists, scores, w.none, n, "ties")
            again = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, output_score=True)
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
            seen = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, exclude_seen=True, output_score=True)
            _assert_rows(seen, w.users, w.lists, scores, w.seen, n, "ties-seen")
            for i in zeros:
                lst = w.lists[i]
                c = min(n, len(lst))
                assert np.array_equal(first[0][i, :c], lst[:c].astype(np.uint64)) and np.all(first[1][i, :c] == 0)
                assert np.all(first[0][i, c:] == api.TOPN_NONE) and np.all(first[1][i, c:] == -np.inf)
                adm = np.setdiff1d(lst, w.seen[i])
                c = min(n, len(adm))
                assert np.array_equal(seen[0][i, :c], adm[:c].astype(np.uint64)) and np.all(seen[0][i, c:] == api.TOPN_NONE)
    finally:
        s.close()


def test_independence_of_company(world, prec):
    """5. a user's row: alone, in its group only, with the batch reversed, with the table's rows permuted, with its group split over
    two calls"""
    w, k, n = world, 50, 10
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    s = _session(w.coo, k, prec, A, B)
    try:
        kw = dict(exclude_seen=True, output_score=True)
        ix_all, sc_all = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, **kw)
        ix_rev, sc_rev = s.topn_batch(w.users[::-1].copy(), n, include=w.incl, include_of=w.of[::-1].copy(), **kw)
        assert np.array_equal(ix_rev[::-1], ix_all) and np.array_equal(sc_rev[::-1], sc_all)
        perm = np.random.default_rng(3).permutation(w.G)                 # new row r of the table is old row perm[r]
        where = np.argsort(perm)
        ix_p, sc_p = s.topn_batch(w.users, n, include=_pair([w.table[g] for g in perm]), include_of=where[w.of], **kw)
        assert np.array_equal(ix_p, ix_all) and np.array_equal(sc_p, sc_all)
        for g in range(w.G):
            members = np.flatnonzero(w.of == g)
            if len(members) == 0:
                continue
            ix_g, sc_g = s.topn_batch(w.users[members], n, include=w.incl, include_of=g, **kw)              # its group only
            assert np.array_equal(ix_g, ix_all[members]) and np.array_equal(sc_g, sc_all[members]), g
            for part in (members[:len(members) // 3], members[len(members) // 3:]):                        # the group over two calls
                ix_h, sc_h = s.topn_batch(w.users[part], n, include=_pair([w.table[g]]), include_of=0, **kw)
                assert np.array_equal(ix_h, ix_all[part]) and np.array_equal(sc_h, sc_all[part]), g
            i = int(members[-1])                                                                           # alone
            ix1, sc1 = s.topn_batch(w.users[i:i + 1], n, include=w.incl, include_of=w.of[i:i + 1], **kw)
            assert np.array_equal(ix1[0], ix_all[i]) and np.array_equal(sc1[0], sc_all[i]), g
    finally:
        s.close()


def test_slices(world, prec):
    """6. 64 users on the full catalogue and on the list of 1000: one or two user tiles, so the lists are cut into slices and merged"""
    w, k = world, 50
    A, B = _factors(DIMA, DIMB, k, prec, 61)
    s = _session(w.coo, k, prec, A, B)
    try:
        users = np.random.default_rng(6).choice(DIMA, 64, replace=False).astype(np.uint64)
        csr = sp.csr_matrix(w.coo)
        csr.sum_duplicates(); csr.sort_indices()
        seen = [csr.indices[csr.indptr[u]:csr.indptr[u + 1]].astype(np.int64) for u in users.astype(np.int64)]
        none = [np.empty(0, np.int64)] * 64
        for ln in (DIMB, 1000):
            g = w.lengths.index(ln)
            lists = [w.table[g]] * 64
            scores = _cell_scores(s, users, lists)
            for n in (10, 128):
                _assert_rows(s.topn_batch(users, n, include=w.incl, include_of=g, output_score=True), users, lists, scores, none, n, f"slices-{ln}")
                _assert_rows(s.topn_batch(users, n, include=w.incl, include_of=g, exclude_seen=True, output_score=True), users, lists, scores, seen,
                             n, f"slices-{ln}-seen")
        # both lists in one call: two tiles whose lists differ in length, one slice length
        of = np.repeat([w.lengths.index(DIMB), w.lengths.index(1000)], 32)
        lists = [w.table[g] for g in of]
        _assert_rows(s.topn_batch(users, 128, include=w.incl, include_of=of, output_score=True), users, lists, _cell_scores(s, users, lists), none, 128,
                     "slices-mixed")
    finally:
        s.close()


def test_chunking():
    """7. 3000 users x 12000 exclusion indices: more than one chunk's exclusion area holds; rows equal those of 64 users at a time"""
    dimA, dimB, k, n, nex = 3000, 25000, 8, 10, 12000
    rng = np.random.default_rng(4)
    coo = sp.coo_matrix((np.ones(30 * dimA), (rng.integers(0, dimA, 30 * dimA), rng.integers(0, dimB, 30 * dimA))), shape=(dimA, dimB))
    A, B = _factors(dimA, dimB, k, True, 8)
    s = _session(coo, k, True, A, B)
    try:
        users = rng.permutation(dimA).astype(np.uint64)
        budget = 256 << 20
        assert dimA * nex > budget // 2 // 4, "the exclusion lists fit one chunk's index area"
        table = [np.arange(dimB), np.sort(rng.choice(dimB, 5000, replace=False)), np.sort(rng.choice(dimB, 300, replace=False))]
        incl = _pair(table)
        of = rng.integers(0, 3, dimA)
        # user at position i: every other item from i % 2 on, shifted by a window of its own
        start = (np.arange(dimA) % 2) + 2 * (np.arange(dimA) % 500)
        ex = (start[:, None] + 2 * np.arange(nex)[None, :]).astype(np.uint64)
        assert int(ex.max()) < dimB
        indptr = np.arange(dimA + 1, dtype=np.uint64) * np.uint64(nex)
        ix, sc = s.topn_batch(users, n, include=incl, include_of=of, exclude_seen=True, exclude=(indptr, ex.reshape(-1)), output_score=True)
        for u0 in range(0, dimA, 64):
            m = min(64, dimA - u0)
            ix1, sc1 = s.topn_batch(users[u0:u0 + m], n, include=incl, include_of=of[u0:u0 + m], exclude_seen=True,
                                    exclude=(indptr[:m + 1], ex[u0:u0 + m].reshape(-1)), output_score=True)
            assert np.array_equal(ix1, ix[u0:u0 + m]) and np.array_equal(sc1, sc[u0:u0 + m]), u0
        csr = sp.csr_matrix(coo)
        csr.sum_duplicates(); csr.sort_indices()
        sample = np.sort(rng.choice(dimA, 32, replace=False))
        lists = [table[of[i]] for i in sample]
        scores = _cell_scores(s, users[sample], lists)
        excl = [np.union1d(csr.indices[csr.indptr[int(users[i])]:csr.indptr[int(users[i]) + 1]], ex[i].astype(np.int64)) for i in sample]
        _assert_rows((ix[sample], sc[sample]), users[sample], lists, scores, excl, n, "chunks")
    finally:
        s.close()


def test_host_pointer_entry_and_model(world, prec):
    """8. poismf_hip_topn_shared / PoisMF.topN_batch(include=table, include_of=...): the session call's rows, bit for bit; include_of
    as a plain int; the scratch is reused"""
    w, k = world, 50
    A, B = _factors(DIMA, DIMB, k, prec, 41)
    s = _session(w.coo, k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        for n in (10, 128):
            a = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, exclude_seen=True, output_score=True)
            a2 = s.topn_batch(w.users, n, include=w.incl, include_of=w.of, exclude_seen=True, output_score=True)   # (same scratch, second call)
            assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
            b = m.topN_batch(w.users, n, exclude=_pair(w.seen), include=w.incl, include_of=w.of, output_score=True)   # (the batch's rows of A only)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        everyone = np.arange(DIMA, dtype=np.uint64)
        g = w.lengths.index(1000)
        X = sp.csr_matrix((np.ones(len(w.incl[1])), w.incl[1].astype(np.int64), w.incl[0].astype(np.int64)), shape=(w.G, DIMB))
        a = s.topn_batch(everyone, 10, include=X, include_of=g, output_score=True)
        b = m.topN_batch(everyone, 10, include=X, include_of=g, output_score=True)                         # (all of A goes up)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = m.topN_batch(everyone, 10, include=w.incl, include_of=np.full(DIMA, g))
        assert np.array_equal(c[0], a[0]) and c[1].size == 0
        e = s.topn_batch(everyone, 10, include=_pair([w.table[g]] * DIMA), output_score=True)              # section 1h, the list per user
        assert np.array_equal(e[0], a[0]) and np.array_equal(e[1], a[1])
        d = s.topn_batch(everyone, 10, output_score=True)   # the dense call after it, in the same scratch
        assert d[0].shape == (DIMA, 10) and np.all(d[1][:, 0] >= a[1][:, 0])
    finally:
        s.close()


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_c_entry_errors_with_a_device(flavour, case):
    """9. rc 2 and nothing written, through the C entry point itself"""
    users, n, table, lof, excl = BAD[case]
    rc, out, sc = _c_shared(flavour, users, n, table, lof, excl)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_valid_call_with_a_device(flavour):
    """9. ... and a valid call in the same process: three lists (one empty, one without a user), a repeated user, exclusions"""
    table = ([0, 3, 3, 9, 11], [7, 8, 9, 0, 1, 2, 3, 4, 5, 20, 21])
    rc, out, sc = _c_shared(flavour, [0, 1, 0, 2], 4, table, [0, 1, 2, 0], ([0, 1, 1, 3, 3], [8, 0, 4]))
    assert rc == 0
    none = -1 if flavour == "r" else api.TOPN_NONE
    # all scores are equal (factors of ones): ascending item indices, the user's exclusions left out, short rows padded
    assert out.tolist() == [[7, 9, none, none], [none] * 4, [1, 2, 3, 5], [7, 8, 9, none]]
    assert sc.tolist() == [[3.0, 3.0, -np.inf, -np.inf], [-np.inf] * 4, [3.0] * 4, [3.0, 3.0, 3.0, -np.inf]]


def test_session_errors_with_a_device(prec):
    """9. the session entry: exclude_seen for a user outside the shard, NULL table / list_of, a list beyond the table: rc 2, nothing
    written, ValueError from the wrapper; valid calls follow"""
    k, dimB = 8, 2000
    rng = np.random.default_rng(3)
    coo = sp.coo_matrix((np.ones(6000), (rng.integers(0, DIMA, 6000), rng.integers(0, dimB, 6000))), shape=(DIMA, dimB))
    csr, csc = harness.process_data(coo, prec)
    A, B = _factors(DIMA, dimB, k, prec, 3)
    s = api.Session(csr, csc, DIMA, dimB, k, prec, shardA=(100, 200), shardB=(0, dimB))
    try:
        s.set_factors(A, B)
        users = np.array([150, 200], np.uint64)
        lp, li, lof = np.array([0, 2, 4], np.uint64), np.array([5, 9, 1, 7], np.uint64), np.array([0, 1], np.uint64)
        out = np.full((2, 5), 12345, np.uint64)
        p = api._ptr
        fn = s.lib.poismf_hip_session_topn_shared
        assert fn(s.h, p(users), 2, 5, p(lp), p(li), 2, p(lof), 1, None, None, p(out), None) == 2     # user 200 is outside the shard
        assert fn(s.h, p(users), 2, 5, None, None, 2, p(lof), 0, None, None, p(out), None) == 2
        assert fn(s.h, p(users), 2, 5, p(lp), p(li), 2, None, 0, None, None, p(out), None) == 2
        assert fn(s.h, p(users), 2, 5, p(lp), p(li), 1, p(lof), 0, None, None, p(out), None) == 2     # list 1 of a table of one
        assert fn(s.h, p(users), 2, 5, p(lp), p(li), 0, p(lof), 0, None, None, p(out), None) == 2
        assert np.all(out == 12345)
        with pytest.raises(ValueError):
            s.topn_batch(users, 5, exclude_seen=True, include=(lp, li), include_of=lof)
        with pytest.raises(ValueError):
            s.topn_batch(users, 5, include=(lp, li), include_of=[0, 2])
        ix, _ = s.topn_batch(users, 5, include=(lp, li), include_of=lof)     # without exclude_seen any user of A may be asked for
        assert sorted(ix[0, :2].tolist()) == [5, 9] and sorted(ix[1, :2].tolist()) == [1, 7] and np.all(ix[:, 2:] == api.TOPN_NONE)
        ix, _ = s.topn_batch([100, 199], 5, exclude_seen=True, include=(lp, li), include_of=1)
        assert ix.shape == (2, 5) and set(ix[:, :2].reshape(-1).tolist()) <= {1, 7, api.TOPN_NONE}
    finally:
        s.close()
