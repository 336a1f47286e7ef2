"""Batched top-N with per-(user, item) score factors (include/poismf_hip.h section 1r) on the GPU: items and score bits against the
existing predict path with the listed cells multiplied by their factors, over depths, exclusions and adjust schemes (cells at the
head of a user's list, cells lifted from far below it, cells sunk to 0, long rows that take several sparse slices, a ragged batch);
the reductions to Session.topn_batch and Session.topn_weighted; exact ties between listed and unlisted items across the two stages
and the item slices; independence of the batch a user is in and of the chunking, the host-pointer entry and the R flavour; and the
shared scratch left usable.

The expectation is built as in tests/test_gpu_topn_deep.py from Session.predict -- the pair_dot_kernel path, which the batched code does
not share: the user's whole score row, its listed cells multiplied by their factors with one numpy multiplication in the model's
precision, minus E(u), ordered by (score descending, item ascending) with np.lexsort, padded with TOPN_NONE and -inf (adjusted_expect;
tests/test_topn_adjusted_cpu.py holds it to hand-written answers).  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_topn_deep import DIMA, DIMB, ZERO_USER, FEW_USER, NONE_USER, _excl_pair, _expect, _factors, _near_the_top, _score_rows, _session
from tests.test_gpu_topn_weighted import same

pytestmark = pytest.mark.gpu

KS = (3, 50, 65)   # 65: two LDS chunks in fp32
DEPTHS = (1, 10, 100, 128)
NO_EXCL = [np.empty(0, np.int64)] * DIMA


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


# ---- the reference ----
def adjusted_rows(score_rows, adj_rows):
    """the score rows with row i's cells adj_rows[i] = (items, factors) multiplied by their factors: one numpy multiplication in the
    rows' own dtype"""
    out = score_rows.copy()
    assert len(adj_rows) == len(score_rows)
    for i, (idx, f) in enumerate(adj_rows):
        idx, f = np.asarray(idx, np.int64), np.asarray(f)
        assert f.shape == idx.shape
        if len(idx):
            assert f.dtype == score_rows.dtype and np.all(np.diff(idx) > 0)
            prod = np.multiply(score_rows[i, idx], f)
            assert prod.dtype == score_rows.dtype
            out[i, idx] = prod
    return out


def adjusted_expect(score_rows, adj_rows, excl, n):
    """[m x n] items and adjusted scores: every row's first n admissible items under (adjusted score descending, item ascending), then
    the padding"""
    return _expect(adjusted_rows(score_rows, adj_rows), excl, n)


def adj_triple(adj_rows, dt):
    """the rows as the (indptr, indices, factors) triple the calls take"""
    indptr = np.zeros(len(adj_rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r[0]) for r in adj_rows])
    idx = np.concatenate([np.asarray(r[0], np.int64) for r in adj_rows]) if len(adj_rows) else np.empty(0, np.int64)
    f = np.concatenate([np.asarray(r[1], dt) for r in adj_rows]) if len(adj_rows) else np.empty(0, dt)
    return indptr, idx.astype(np.uint64), f.astype(dt)


def _sub(adj_rows, users):
    return [adj_rows[int(u)] for u in users]


EMPTY = lambda dt: (np.empty(0, np.int64), np.empty(0, dt))


# ---- adjust schemes: name -> one (items, factors) row per user ----
def _schemes(A, B, dt, seed):
    rng = np.random.default_rng(seed)
    approx = A.astype(np.float64) @ B.astype(np.float64).T
    order = np.argsort(-approx, axis=1, kind="stable")        # (which items these are exactly does not matter)
    head = [np.sort(r) for r in order[:, :200:2]]
    long = [(np.sort(rng.choice(DIMB, 2500, replace=False)), rng.uniform(0.9, 1.1, 2500).astype(dt)) for _ in range(DIMA)]
    return {
        "mixed": [(c, rng.uniform(0.95, 1.05, len(c)).astype(dt)) for c in head],
        "head": [(c, np.exp(rng.uniform(np.log(1 / 8), np.log(8.0), len(c))).astype(dt)) for c in head],
        "lift": [(np.sort(rng.choice(order[i, -1000:], 20, replace=False)), np.full(20, 1024, dt)) for i in range(DIMA)],
        "sink": [(np.sort(order[i, :30]), np.zeros(30, dt)) for i in range(DIMA)],
        "long": long,
        "ragged": [long[i] if i % 3 == 0 else EMPTY(dt) for i in range(DIMA)],
    }


def _model(A, B, k, prec):
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, A.shape[0], B.shape[0], True
    return m


@pytest.mark.parametrize("k", KS)
def test_bits_against_the_predict_path(prec, k):
    """every depth x {no exclusion, exclude_seen, a batch list} x every adjust scheme; the excluded items come from the top of the user's
    plain list and overlap the listed cells; one user keeps 5 items, one keeps none (both with listed cells among the excluded ones),
    one row of A is zero (every adjusted score 0: the smallest indices)"""
    A, B = _factors(DIMA, DIMB, k, prec, 500 + k)
    A[ZERO_USER] = 0
    rng = np.random.default_rng(k)
    seen = _near_the_top(A, B, 3, 300)
    extra = _near_the_top(A, B, 5, 300)
    everything = np.arange(DIMB)
    seen[FEW_USER + 4] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))
    seen[NONE_USER + 4] = everything
    extra[FEW_USER] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))
    extra[NONE_USER] = everything
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, users, DIMB)
        assert not rows[ZERO_USER].any()
        tiny = np.finfo(rows.dtype).tiny
        excl = {"plain": NO_EXCL, "seen": seen, "list": extra}
        kwargs = {"plain": {}, "seen": {"exclude_seen": True}, "list": {"exclude": _excl_pair(extra)}}
        plain_all = _expect(rows, NO_EXCL, DIMB)[0].astype(np.int64)
        place = np.empty((DIMA, DIMB), np.int64)                      # place[u, j]: item j's place in user u's plain order
        np.put_along_axis(place, plain_all, np.arange(DIMB)[None, :], axis=1)
        plain10 = s.topn_batch(users, 10)[0]
        assert np.array_equal(plain10.astype(np.int64), plain_all[:, :10])
        others = np.setdiff1d(np.arange(DIMA), [ZERO_USER])
        for name, adj in _schemes(A, B, rows.dtype, 7 * k).items():
            adjusted = adjusted_rows(rows, adj)
            assert adjusted[adjusted > 0].min() > tiny                # no positive product is denormal
            triple = adj_triple(adj, rows.dtype)
            for how in excl:
                want = _expect(adjusted, excl[how], max(DEPTHS))
                if how == "plain":
                    top = want[0][:, :10].astype(np.int64)
                    listed = np.array([np.isin(top[i], adj[i][0]) for i in range(DIMA)])
                    if name == "mixed":
                        both = int((listed.any(axis=1) & ~listed.all(axis=1)).sum())
                        print(f"k {k} mixed: a listed and an unlisted item in the top 10 of {both} of {DIMA} users")
                        assert 2 * both >= DIMA                       # the merge of the two stages is exercised
                    if name == "head":
                        differ = int((want[0][:, :10] != plain10).any(axis=1).sum())
                        print(f"k {k} head: the factors change the top 10 of {differ} of {DIMA} users")
                        assert 2 * differ >= DIMA                     # a kernel that ignores the factors cannot pass
                    if name == "lift":
                        deep = np.take_along_axis(place, top, axis=1).max(axis=1)
                        print(f"k {k} lift: the deepest plain place in a top 10 is at least {int(deep[others].min())}")
                        # every row but the zero row of A, whose scores no factor moves: no re-rank of topn_deep's 1024 finds these
                        assert np.all(deep[others] >= 1024)
                    if name == "sink":
                        assert not listed[others].any()               # the best 30 fell to 0 and left the top
                    assert want[0][ZERO_USER].tolist() == list(range(max(DEPTHS)))   # all ties at 0: index order
                if how == "list":
                    assert (want[0][FEW_USER] != api.TOPN_NONE).sum() == 5 and (want[0][NONE_USER] == api.TOPN_NONE).all()
                    if name != "ragged":                              # (there FEW_USER's row is empty) listed cells among the excluded ones
                        assert len(np.intersect1d(adj[FEW_USER][0], extra[FEW_USER])) and len(adj[NONE_USER][0])
                for n in DEPTHS:
                    same(s.topn_adjusted(users, n, adjust=triple, output_score=True, **kwargs[how]), want, f"{name} n {n} {how}", n)
        ix, sc = s.topn_adjusted(users, 10, adjust=triple)
        assert np.array_equal(ix, adjusted_expect(rows, adj, NO_EXCL, 10)[0]) and sc.size == 0
        # the lift scheme once more on the factors as drawn, without the zero row of A (whose scores no factor moves): EVERY row's top
        # 10 holds an item from beyond place 1024 of its plain order
        A_full = _factors(DIMA, DIMB, k, prec, 500 + k)[0]
        s.set_factors(A_full, B)
        rows = _score_rows(s, users, DIMB)
        lift = _schemes(A_full, B, rows.dtype, 7 * k)["lift"]
        plain_all = _expect(rows, NO_EXCL, DIMB)[0].astype(np.int64)
        np.put_along_axis(place, plain_all, np.arange(DIMB)[None, :], axis=1)
        want = adjusted_expect(rows, lift, NO_EXCL, max(DEPTHS))
        deep = np.take_along_axis(place, want[0][:, :10].astype(np.int64), axis=1).max(axis=1)
        print(f"k {k} lift, no zero row: the deepest plain place in a top 10 is at least {int(deep.min())} over all {DIMA} users")
        assert np.all(deep >= 1024)
        for n in (10, 128):
            same(s.topn_adjusted(users, n, adjust=adj_triple(lift, rows.dtype), output_score=True), want, f"lift, no zero row n {n}", n)
    finally:
        s.close()


def test_long_rows_many_slices_and_cells_lost_to_the_exclusion(prec):
    """110 000 items, five users: a row of 104 449 cells that loses one cell to the exclusion list -- at n = 10 the row as given would
    take 97 work items and the row that is left takes 102, slices of 1088 and 1024 cells, with 102 item slices beside them: every list
    the merge can rank -- next to an empty row, a row of 30 000 cells, one of 5 and one of 2000; n = 128: 8 slices of 13 056 cells"""
    k, dimA, dimB = 3, 5, 110000
    dt = H.dtype_of(prec)
    A, B = _factors(dimA, dimB, k, prec, 61)
    rng = np.random.default_rng(62)
    lens = (104449, 0, 30000, 5, 2000)
    adj = [(np.sort(rng.choice(dimB, c, replace=False)), np.exp(rng.uniform(np.log(0.5), np.log(2.0), c)).astype(dt)) for c in lens]
    excl = [np.array([adj[0][0][50000], dimB - 1]), np.empty(0, np.int64), adj[2][0][::3], np.empty(0, np.int64), np.arange(0, dimB, 2)]
    excl[0].sort()
    lib = api.load_library(prec)
    assert int(lib.poismf_hip_topn_adjusted_slices(104449, 10, 0)) == 97 and int(lib.poismf_hip_topn_adjusted_slices(104448, 10, 0)) == 102
    assert int(lib.poismf_hip_topn_adjusted_slices(104448, 128, 0)) == 8
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        users = np.arange(dimA, dtype=np.uint64)
        rows = _score_rows(s, users, dimB)
        triple = adj_triple(adj, dt)
        for n in (10, 128):
            same(s.topn_adjusted(users, n, adjust=triple, exclude=_excl_pair(excl), output_score=True), adjusted_expect(rows, adj, excl, n), f"long rows n {n}")
            same(s.topn_adjusted(users, n, adjust=triple, output_score=True), adjusted_expect(rows, adj, [[]] * dimA, n), f"long rows, nothing excluded n {n}")
        one = s.topn_adjusted(users[:1], 10, adjust=adj_triple(adj[:1], dt), exclude=_excl_pair(excl[:1]), output_score=True)
        same(one, adjusted_expect(rows[:1], adj[:1], excl[:1], 10), "the long row alone")
    finally:
        s.close()


def test_reductions(prec):
    """nothing listed, and every factor 1 on the head cells: Session.topn_batch's rows bit for bit; every item listed with factor w[j]:
    Session.topn_weighted's; every factor 0.5 on every item: the plain items, scores halved; a cell listed and excluded is absent"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 23)
    dt = H.dtype_of(prec)
    seen = _near_the_top(A, B, 3, 100)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        head = _near_the_top(A, B, 2, 200)
        ones = adj_triple([(c, np.ones(len(c), dt)) for c in head], dt)
        nothing = (np.zeros(DIMA + 1, np.uint64), np.empty(0, np.uint64), np.empty(0, dt))
        every = np.arange(DIMB)
        w = np.exp(np.random.default_rng(6).uniform(np.log(0.25), np.log(4.0), DIMB)).astype(dt)
        w[::7] = 0
        full = adj_triple([(every, w)] * DIMA, dt)
        halves = adj_triple([(every, np.full(DIMB, 0.5, dt))] * DIMA, dt)
        for n in (1, 10, 128):
            plain = s.topn_batch(users, n, exclude_seen=True, output_score=True)
            same(s.topn_adjusted(users, n, adjust=None, exclude_seen=True, output_score=True), plain, f"adjust None n {n}")
            same(s.topn_adjusted(users, n, adjust=nothing, exclude_seen=True, output_score=True), plain, f"nothing listed n {n}")
            same(s.topn_adjusted(users, n, adjust=sp.csr_matrix((DIMA, DIMB)), exclude_seen=True, output_score=True), plain, f"an empty matrix n {n}")
            same(s.topn_adjusted(users, n, adjust=ones, exclude_seen=True, output_score=True), plain, f"factors of one n {n}")
            weighted = s.topn_weighted(users, n, item_weight=w, exclude_seen=True, output_score=True)
            same(s.topn_adjusted(users, n, adjust=full, exclude_seen=True, output_score=True), weighted, f"every item listed n {n}")
            halved = plain[0], np.multiply(plain[1], plain[1].dtype.type(0.5))
            same(s.topn_adjusted(users, n, adjust=halves, exclude_seen=True, output_score=True), halved, f"one half everywhere n {n}")
        # the head cells boosted eightfold and excluded: none of them comes back, and the rows are the plain call's with that list
        boost = adj_triple([(c, np.full(len(c), 8, dt)) for c in head], dt)
        pair = _excl_pair(head)
        got = s.topn_adjusted(users, 10, adjust=boost, exclude=pair, output_score=True)
        assert not any(np.isin(got[0][i].astype(np.int64), head[i]).any() for i in range(DIMA))
        same(got, s.topn_batch(users, 10, exclude=pair, output_score=True), "listed and excluded")
        got = s.topn_adjusted(users, 10, adjust=boost, exclude_seen=True, output_score=True)
        assert not any(np.isin(got[0][i].astype(np.int64), seen[i]).any() for i in range(DIMA))
        assert all(np.isin(got[0][i].astype(np.int64), head[i]).all() for i in range(DIMA))   # (the boosted cells that are left lead)
    finally:
        s.close()


def test_ties_across_the_stages_and_the_slices(prec):
    """integer factors and cell factors that are powers of two: every product is exact, and listed and unlisted items tie exactly.  The
    index order must hold across the two stages, across item slices (five users: many of them) and across the two sparse slices of a
    row of 1500 cells"""
    k = 50
    dt = H.dtype_of(prec)
    rng = np.random.default_rng(29)
    A, B = rng.integers(0, 4, (DIMA, k)).astype(dt), rng.integers(0, 4, (DIMB, k)).astype(dt)
    # (few cells are doubled: they lead every list; behind them listed cells at factor 1 or halved and unlisted ones share the integers)
    adj = [(np.sort(rng.choice(DIMB, 1500, replace=False)), rng.choice([0.5, 1.0, 2.0], 1500, p=[0.3, 0.68, 0.02]).astype(dt)) for _ in range(DIMA)]
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, everyone, DIMB)
        assert np.array_equal(rows, (A.astype(np.float64) @ B.astype(np.float64).T).astype(dt))   # integers: exact in any order
        few = np.array([0, 64, 129, 5, 77], np.uint64)
        for n in (10, 100, 128):
            want = adjusted_expect(rows, adj, NO_EXCL, n)
            same(s.topn_adjusted(everyone, n, adjust=adj_triple(adj, dt), output_score=True), want, f"130 users n {n}")
            f = few.astype(np.int64)
            same(s.topn_adjusted(few, n, adjust=adj_triple(_sub(adj, few), dt), output_score=True), (want[0][f], want[1][f]), f"five users n {n}")
        met = 0   # neighbours in a top 128 that tie, one of them listed and the other not
        for i in range(DIMA):
            listed = np.isin(want[0][i].astype(np.int64), adj[i][0])
            met += int(((want[1][i][1:] == want[1][i][:-1]) & (listed[1:] != listed[:-1])).sum())
        print(f"ties between a listed and an unlisted neighbour in a top 128: {met}")
        assert met >= DIMA
    finally:
        s.close()


def test_invariance_host_pointers_and_the_r_flavour(prec):
    """a user alone, in the shuffled batch of 130, repeated within a batch, and in a batch whose adjust cells take several chunks: the
    same row; PoisMF.topN_adjusted (host pointers; a SciPy matrix and the triple) and, in double, the R flavour through ctypes: the
    session's rows, bit for bit; a topn_batch before and after gives the same rows (the calls share the session's scratch)"""
    k, n = 50, 20
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    dt = H.dtype_of(prec)
    seen = _near_the_top(A, B, 3, 300)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    m = _model(A, B, k, prec)
    rng = np.random.default_rng(2)
    adj = [(np.sort(rng.choice(DIMB, 2200, replace=False)), np.exp(rng.uniform(np.log(0.25), np.log(4.0), 2200)).astype(dt)) for _ in range(DIMA)]
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        before = s.topn_batch(everyone, 10, exclude_seen=True, output_score=True)
        call = lambda u: s.topn_adjusted(u, n, adjust=adj_triple(_sub(adj, u), dt), exclude_seen=True, output_score=True)
        ix_all, sc_all = call(everyone)
        same((ix_all, sc_all), adjusted_expect(_score_rows(s, everyone, DIMB), adj, seen, n), "130 users")
        perm = np.random.default_rng(3).permutation(DIMA)
        ix_p, sc_p = call(everyone[perm])
        assert np.array_equal(ix_p, ix_all[perm]) and sc_p.tobytes() == sc_all[perm].tobytes()
        for u in (0, 63, 64, 129):
            ix1, sc1 = call([u])
            ix5, sc5 = call([u, 11, u, 100, u])
            for p in (0, 2, 4):
                assert np.array_equal(ix5[p], ix_all[u]) and sc5[p].tobytes() == sc_all[u].tobytes()
            assert np.array_equal(ix1[0], ix_all[u]) and sc1[0].tobytes() == sc_all[u].tobytes()
        # 2000 users x 2200 cells: more cells than one chunk's adjust area holds, so the batch is cut into several chunks
        many = np.tile(everyone, 2000 // DIMA + 1)[:2000]
        big = adj_triple(_sub(adj, many), dt)
        assert len(big[1]) > api.TOPN_ADJUSTED_MAX_ROW, "the batch does not exceed one chunk's adjust area"
        ix_m, sc_m = s.topn_adjusted(many, n, adjust=big, exclude_seen=True, output_score=True)
        mm = many.astype(np.int64)
        assert np.array_equal(ix_m, ix_all[mm]) and sc_m.tobytes() == sc_all[mm].tobytes()
        after = s.topn_batch(everyone, 10, exclude_seen=True, output_score=True)
        assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()

        users = np.array([3, 129, 64, 3, 77, 0], np.uint64)
        pair = _excl_pair([seen[u] for u in users])
        triple = adj_triple(_sub(adj, users), dt)
        a = call(users)
        b = m.topN_adjusted(users, n, adjust=triple, exclude=pair, output_score=True)   # (the batch's rows of A only)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        mat = sp.csr_matrix((triple[2], triple[1].astype(np.int64), triple[0].astype(np.int64)), shape=(len(users), DIMB))
        b = m.topN_adjusted(users, n, adjust=mat, exclude=pair, output_score=True)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        pair_all, triple_all = _excl_pair(seen), adj_triple(adj, dt)
        c = m.topN_adjusted(everyone, n, adjust=triple_all, exclude=pair_all, output_score=True)   # (all of A goes up)
        assert np.array_equal(c[0], ix_all) and c[1].tobytes() == sc_all.tobytes()
        if not prec:
            lib = api.load_library("r")
            i32 = lambda v: np.ascontiguousarray(np.asarray(v, np.uint64).astype(np.int32))
            u, ip, ii, ap, ai = i32(everyone), i32(pair_all[0]), i32(pair_all[1]), i32(triple_all[0]), i32(triple_all[1])
            out, sc = np.zeros((DIMA, n), np.int32), np.zeros((DIMA, n), np.float64)
            p = api._ptr
            rc = lib.poismf_hip_topn_adjusted(p(A), p(B), k, DIMA, DIMB, p(u), DIMA, n, p(ap), p(ai), p(triple_all[2]), p(ip), p(ii), p(out), p(sc))
            assert rc == 0
            assert np.array_equal(out.astype(np.int64).astype(np.uint64), ix_all) and sc.tobytes() == sc_all.tobytes()
    finally:
        s.close()


def test_the_model_call_discounts_the_seen_items(prec):
    """PoisMF.topN_adjusted with the users' own rows of X as the adjust list, every stored value set to 0.5 -- seen items discounted,
    not barred: the session's rows, and the reference's"""
    k, n = 50, 10
    A, B = _factors(DIMA, DIMB, k, prec, 88)
    seen = _near_the_top(A, B, 2, 40)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.array([5, 0, 129, 64, 5, 100, 17], np.uint64)
        row = np.concatenate([np.full(len(r), i) for i, r in enumerate(seen)])
        X = sp.csr_matrix((np.ones(len(row)), (row, np.concatenate(seen))), shape=(DIMA, DIMB))
        adj = X[users.astype(np.int64)].copy()
        adj.data[:] = 0.5
        got = _model(A, B, k, prec).topN_adjusted(users, n, adjust=adj, output_score=True)
        same(got, s.topn_adjusted(users, n, adjust=adj, output_score=True), "model against session")
        dt = H.dtype_of(prec)
        rows = [(seen[int(u)], np.full(len(seen[int(u)]), 0.5, dt)) for u in users]
        want = adjusted_expect(_score_rows(s, users, DIMB), rows, [[]] * len(users), n)
        same(got, want, "model against the reference")
    finally:
        s.close()
