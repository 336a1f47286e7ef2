"""Batched top-N with per-item score weights and the cosine similar-items call on top of it (include/poismf_hip.h section 1o) on the
GPU: items and score bits against the existing predict path times the weights, over depths, exclusions and weight schemes (with
weight-0 items); the reductions to Session.topn_batch; all-tie rows and ties across item slices; short and empty rows; independence of
the batch a user is in, the host-pointer entry and the R flavour; rows of B as the queries; similar_items on both classes; and the
shared scratch left usable.

The expectation is built as in tests/test_gpu_topn_deep.py from Session.predict -- the pair_dot_kernel path, which the batched code does
not share: the user's whole score row, multiplied by the weights with numpy in the model's precision, minus E(u), ordered by (weighted
score descending, item ascending) with np.lexsort, padded with TOPN_NONE and -inf (weighted_expect; tests/test_topn_weighted_cpu.py
holds it to hand-written answers).  There is no tolerance anywhere in this file."""
import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_topn_deep import DIMA, DIMB, ZERO_USER, FEW_USER, NONE_USER, _excl_pair, _factors, _near_the_top, _score_rows, _session

pytestmark = pytest.mark.gpu

KS = (3, 50, 65)   # 65: two LDS chunks in fp32
DEPTHS = (1, 10, 100, 128)
NO_EXCL = [np.empty(0, np.int64)] * DIMA


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


# ---- the reference ----
def weighted_expect(score_rows, weight, excl, n):
    """[m x n] items and weighted scores: every row of scores times the weights (one numpy multiplication in the rows' own dtype), its
    first n admissible items under (weighted score descending, item ascending), then the padding"""
    weight = np.asarray(weight)
    assert weight.dtype == score_rows.dtype and weight.shape == (score_rows.shape[1],)
    w = np.multiply(score_rows, weight[None, :])
    assert w.dtype == score_rows.dtype
    m, dimB = w.shape
    ix = np.full((m, n), api.TOPN_NONE, np.uint64)
    sc = np.full((m, n), -np.inf, w.dtype)
    for i in range(m):
        idx = np.setdiff1d(np.arange(dimB), np.asarray(excl[i], np.int64))
        s = w[i, idx]
        o = np.lexsort((idx, -s.astype(np.float64)))[:n]   # (the cast is exact; it only keeps -s in one dtype)
        ix[i, :len(o)] = idx[o]
        sc[i, :len(o)] = s[o]
    return ix, sc


def same(got, want, what, n=None):
    """got [m x n] against the first n columns of want (a row's padding starts where its admissible items end, at every n)"""
    if n is not None:
        want = want[0][:, :n], np.ascontiguousarray(want[1][:, :n])
    ok_ix, ok_sc = np.array_equal(got[0], want[0]), got[1].tobytes() == want[1].tobytes()
    print(f"{what}: equal ix {ok_ix} equal score bits {ok_sc}")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    if not ok_ix:
        bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
        raise AssertionError((what, "rows", bad[:8].tolist(), got[0][bad[0]][:12], want[0][bad[0]][:12]))
    assert ok_sc, what


# ---- weight schemes: name -> [dimB] weights in the model's precision ----
def _schemes(dimB, dt, seed):
    rng = np.random.default_rng(seed)
    half = rng.uniform(0.5, 2.0, dimB)
    half[rng.permutation(dimB)[:dimB // 2]] = 0.0
    return {
        "log-uniform": np.exp(rng.uniform(np.log(0.25), np.log(4.0), dimB)).astype(dt),
        "near-one": rng.uniform(0.9, 1.1, dimB).astype(dt),
        "half-zero": half.astype(dt),
        "powers-of-two": rng.choice([0.5, 1.0, 2.0], dimB).astype(dt),
    }


def _model(A, B, k, prec):
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, A.shape[0], B.shape[0], True
    return m


@pytest.mark.parametrize("k", KS)
def test_bits_against_the_predict_path(prec, k):
    """every depth x {no exclusion, exclude_seen, a batch list} x every weight scheme; the excluded items come from the top of the user's
    unweighted list; one user keeps 5 items, one keeps none, one row of A is zero (every weighted score 0: the smallest indices)"""
    A, B = _factors(DIMA, DIMB, k, prec, 500 + k)
    A[ZERO_USER] = 0
    rng = np.random.default_rng(k)
    seen = _near_the_top(A, B, 2, 200)
    extra = _near_the_top(A, B, 3, 300)
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
        excl = {"plain": NO_EXCL, "seen": seen, "list": extra}
        kwargs = {"plain": {}, "seen": {"exclude_seen": True}, "list": {"exclude": _excl_pair(extra)}}
        plain10 = s.topn_batch(users, 10)[0]
        for name, w in _schemes(DIMB, rows.dtype, 7 * k).items():
            positive = np.multiply(rows, w[None, :])
            positive = positive[positive > 0]
            assert positive.min() > np.finfo(rows.dtype).tiny        # no product is denormal
            for how in excl:
                want = weighted_expect(rows, w, excl[how], max(DEPTHS))
                if how == "plain":
                    differ = int((want[0][:, :10] != plain10).any(axis=1).sum())
                    print(f"k {k} {name}: the weights change the top 10 of {differ} of {DIMA} users")
                    assert 2 * differ >= DIMA                        # a kernel that ignores the weights cannot pass
                    assert want[0][ZERO_USER].tolist() == list(range(max(DEPTHS)))
                if how == "list":
                    assert (want[0][FEW_USER] != api.TOPN_NONE).sum() == 5 and (want[0][NONE_USER] == api.TOPN_NONE).all()
                for n in DEPTHS:
                    same(s.topn_weighted(users, n, item_weight=w, output_score=True, **kwargs[how]), want, f"{name} n {n} {how}", n)
        ix, sc = s.topn_weighted(users, 10, item_weight=w)
        assert np.array_equal(ix, weighted_expect(rows, w, NO_EXCL, 10)[0]) and sc.size == 0
    finally:
        s.close()


def test_reductions_to_the_plain_call(prec):
    """every weight 1 (an array, and the scalar): Session.topn_batch's rows bit for bit; every weight 0.5: the same items, scores halved"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 23)
    seen = _near_the_top(A, B, 2, 100)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        ones = np.ones(DIMB, H.dtype_of(prec))
        for n in (1, 10, 128):
            plain = s.topn_batch(users, n, exclude_seen=True, output_score=True)
            same(s.topn_weighted(users, n, item_weight=ones, exclude_seen=True, output_score=True), plain, f"ones n {n}")
            same(s.topn_weighted(users, n, item_weight=1, exclude_seen=True, output_score=True), plain, f"scalar one n {n}")
            halved = plain[0], np.multiply(plain[1], plain[1].dtype.type(0.5))
            same(s.topn_weighted(users, n, item_weight=0.5, exclude_seen=True, output_score=True), halved, f"one half n {n}")
    finally:
        s.close()


def test_ties_within_and_across_slices(prec):
    """factors of ones: every score is k, so the order is weight class descending, then index ascending, across item slices; 200 rows of
    B repeated 1600 indices apart with equal weights: the twins tie and the smaller index comes first.  Few users: many item slices and
    the merge; 768 x 64 entries that repeat the 130 rows: one slice, no merge"""
    k = 50
    dt = H.dtype_of(prec)
    s = _session(DIMA, DIMB, k, prec, np.ones((DIMA, k), dt), np.ones((DIMB, k), dt))
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        w = np.random.default_rng(5).choice([0.5, 1.0, 2.0], DIMB).astype(dt)
        rows = _score_rows(s, everyone, DIMB)
        assert np.all(rows == k)
        for n in (10, 128):
            want = weighted_expect(rows, w, NO_EXCL, n)
            assert want[0][0].tolist() == np.flatnonzero(w == 2.0)[:n].tolist()
            same(s.topn_weighted(everyone, n, item_weight=w, output_score=True), want, f"all ties n {n}")
            same(s.topn_weighted(everyone[:5], n, item_weight=w, output_score=True), (want[0][:5], want[1][:5]), f"all ties, 5 users n {n}")
    finally:
        s.close()

    A, B = _factors(DIMA, DIMB, k, prec, 91)
    rng = np.random.default_rng(17)
    src = rng.choice(1400, 200, replace=False)
    dst = src + 1600
    B[dst] = B[src]
    w = _schemes(DIMB, dt, 3)["log-uniform"]
    w[dst] = w[src]
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        rows = _score_rows(s, everyone, DIMB)
        assert np.array_equal(rows[:, dst], rows[:, src])
        few = np.array([0, 64, 129, 5, 77], np.uint64)
        for n in (10, 100, 128):
            want = weighted_expect(rows, w, NO_EXCL, n)
            got = s.topn_weighted(few, n, item_weight=w, output_score=True)
            same(got, (want[0][few.astype(np.int64)], want[1][few.astype(np.int64)]), f"few users n {n}")
            same(s.topn_weighted(everyone, n, item_weight=w, output_score=True), want, f"130 users n {n}")
        pairs = {int(a): int(b) for a, b in zip(src, dst)}
        met = sum(1 for row in want[0] for p in range(127) if pairs.get(int(row[p])) == int(row[p + 1]))
        print(f"twins next to each other in a top 128: {met}")
        assert met > 0
        want = weighted_expect(rows, w, NO_EXCL, 10)
        many = np.tile(everyone, 768 * 64 // DIMA + 1)[:768 * 64]
        ix, sc = s.topn_weighted(many, 10, item_weight=w, output_score=True)
        same((ix[:DIMA], sc[:DIMA]), want, "one slice")
        m = many.astype(np.int64)
        assert np.array_equal(ix, ix[:DIMA][m]) and sc.tobytes() == sc[:DIMA][m].tobytes()   # every repeat equals the first occurrence
    finally:
        s.close()


def test_one_item_tile(prec):
    """dimB = 40: one tile of items, 24 of its columns past the end; n = 10 and n = 40 (everything listed, or all but the seen item)"""
    k, dimB = 7, 40
    A, B = _factors(DIMA, dimB, k, prec, 4)
    s = _session(DIMA, dimB, k, prec, A, B)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, users, dimB)
        w = _schemes(dimB, rows.dtype, 1)["half-zero"]
        seen = [np.array([i % dimB]) for i in range(DIMA)]
        for n in (10, 40):
            same(s.topn_weighted(users, n, item_weight=w, output_score=True), weighted_expect(rows, w, NO_EXCL, n), f"40 items n {n}")
            got = s.topn_weighted(users, n, item_weight=w, exclude_seen=True, output_score=True)
            same(got, weighted_expect(rows, w, seen, n), f"40 items, seen n {n}")
        assert np.all(got[0][:, 39] == api.TOPN_NONE) and np.all(got[0][:, :39] != api.TOPN_NONE)
    finally:
        s.close()


def test_short_and_empty_rows_list_weight_zero_items(prec):
    """a user who keeps 5 items, 3 of them at weight 0: the 2 others first, then the 3 at score 0 in index order, then the padding; a
    user who keeps none: all padding"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 31)
    dt = H.dtype_of(prec)
    w = _schemes(DIMB, dt, 9)["half-zero"]
    zero, pos = np.flatnonzero(w == 0), np.flatnonzero(w > 0)
    kept = np.sort(np.r_[zero[[3, 700, 1500]], pos[[10, 900]]])
    excl = [np.empty(0, np.int64)] * DIMA
    excl[FEW_USER] = np.setdiff1d(np.arange(DIMB), kept)
    excl[NONE_USER] = np.arange(DIMB)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, users, DIMB)
        for sub in (users, users[[FEW_USER, NONE_USER, 3]]):       # (many users: few slices; three users: many slices and the merge)
            e = [excl[int(u)] for u in sub]
            for n in (1, 10, 128):
                want = weighted_expect(rows[sub.astype(np.int64)], w, e, n)
                got = s.topn_weighted(sub, n, item_weight=w, exclude=_excl_pair(e), output_score=True)
                same(got, want, f"{len(sub)} users n {n}")
        few = got[0][0].tolist(), got[1][0].tolist()
        assert set(few[0][:2]) == set(pos[[10, 900]].tolist()) and few[0][2:5] == zero[[3, 700, 1500]].tolist()
        assert few[1][2:5] == [0.0] * 3 and min(few[1][:2]) > 0
        assert few[0][5:] == [api.TOPN_NONE] * 123 and few[1][5:] == [-np.inf] * 123
        assert np.all(got[0][1] == api.TOPN_NONE) and np.all(got[1][1] == -np.inf)
    finally:
        s.close()


def test_independence_host_pointers_and_the_r_flavour(prec):
    """a user alone, in a batch of 5, in the shuffled batch of 130 and repeated within a batch: the same row; PoisMF.topN_weighted (host
    pointers) and, in double, the R flavour through ctypes: the session's rows, bit for bit"""
    k, n = 50, 20
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    seen = _near_the_top(A, B, 2, 200)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    m = _model(A, B, k, prec)
    w = _schemes(DIMB, H.dtype_of(prec), 2)["log-uniform"]
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        call = lambda u: s.topn_weighted(u, n, item_weight=w, exclude_seen=True, output_score=True)
        ix_all, sc_all = call(everyone)
        perm = np.random.default_rng(3).permutation(DIMA)
        ix_p, sc_p = call(everyone[perm])
        assert np.array_equal(ix_p, ix_all[perm]) and sc_p.tobytes() == sc_all[perm].tobytes()
        for u in (0, 63, 64, 129):
            ix1, sc1 = call([u])
            ix5, sc5 = call([u, 11, u, 100, u])
            for p in (0, 2, 4):
                assert np.array_equal(ix5[p], ix_all[u]) and sc5[p].tobytes() == sc_all[u].tobytes()
            assert np.array_equal(ix1[0], ix_all[u]) and sc1[0].tobytes() == sc_all[u].tobytes()
        users = np.array([3, 129, 64, 3, 77, 0], np.uint64)
        pair = _excl_pair([seen[u] for u in users])
        a = call(users)
        b = m.topN_weighted(users, n, item_weight=w, exclude=pair, output_score=True)   # (the batch's rows of A only)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        pair_all = _excl_pair(seen)
        c = m.topN_weighted(everyone, n, item_weight=w, exclude=pair_all, output_score=True)   # (all of A goes up)
        assert np.array_equal(c[0], ix_all) and c[1].tobytes() == sc_all.tobytes()
        if not prec:
            lib = api.load_library("r")
            i32 = lambda v: np.ascontiguousarray(np.asarray(v, np.uint64).astype(np.int32))
            u, ip, ii = i32(everyone), i32(pair_all[0]), i32(pair_all[1])
            out, sc = np.zeros((DIMA, n), np.int32), np.zeros((DIMA, n), np.float64)
            p = api._ptr
            rc = lib.poismf_hip_topn_weighted(p(A), p(B), k, DIMA, DIMB, p(u), DIMA, n, p(w), p(ip), p(ii), p(out), p(sc))
            assert rc == 0
            assert np.array_equal(out.astype(np.int64).astype(np.uint64), ix_all) and sc.tobytes() == sc_all.tobytes()
    finally:
        s.close()


def _item_rows(B, items):
    """the score rows of rows `items` of B against all of B from predict_multiple with B in both factor arguments"""
    items = np.asarray(items, np.uint64)
    dimB = B.shape[0]
    out = np.empty(len(items) * dimB, B.dtype)
    api._predict_multiple(out, B, B, np.repeat(items, dimB), np.tile(np.arange(dimB, dtype=np.uint64), len(items)))
    return out.reshape(len(items), dimB)


def test_rows_of_b_as_the_queries(prec):
    """query_items=True: the queries are rows of the resident B, also those with indices from DIMA on"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 41)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        items = np.array([0, 1, 129, 130, 131, 2000, 3076, 64, 1, 1500] + list(range(140, 200)), np.uint64)   # 70 queries
        assert len(items) % 64 and items.max() >= DIMA
        rows = _item_rows(B, items)
        w = _schemes(DIMB, rows.dtype, 6)["log-uniform"]
        own = [np.array([int(i)]) for i in items]
        for n in (10, 128):
            same(s.topn_weighted(items, n, item_weight=w, output_score=True, query_items=True), weighted_expect(rows, w, [[]] * len(items), n),
                 f"rows of B n {n}")
            same(s.topn_weighted(items, n, item_weight=w, exclude=_excl_pair(own), output_score=True, query_items=True),
                 weighted_expect(rows, w, own, n), f"rows of B, self excluded n {n}")
        with pytest.raises(ValueError, match="exclude_seen"):
            s.topn_weighted(items, 10, item_weight=w, exclude_seen=True, query_items=True)
        with pytest.raises(ValueError, match="out of range"):
            s.topn_weighted([0, DIMB], 10, item_weight=w, query_items=True)
        with pytest.raises(ValueError, match="out of range"):
            s.topn_weighted([0, DIMA], 10, item_weight=w)                 # (a user, not an item)
        u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
        out = np.full((2, 10), 12345, np.uint64)
        p = api._ptr
        assert s.lib.poismf_hip_session_topn_weighted(s.h, p(u64([0, DIMB])), 2, 10, p(w), 1, 0, None, None, p(out), None) == 2
        assert s.lib.poismf_hip_session_topn_weighted(s.h, p(u64([0, 1])), 2, 10, p(w), 1, 1, None, None, p(out), None) == 2
        assert np.all(out == 12345)
    finally:
        s.close()


def _similar_expect(B, items, n, exclude_self):
    """section 1o's cosine reduction rebuilt from predict bits"""
    dimB = B.shape[0]
    every = np.arange(dimB, dtype=np.uint64)
    n2 = np.empty(dimB, B.dtype)
    api._predict_multiple(n2, B, B, every, every)
    inv = np.zeros(dimB, B.dtype)
    nz = n2 != 0
    inv[nz] = B.dtype.type(1) / np.sqrt(n2[nz])
    assert inv.dtype == B.dtype
    excl = [[int(i)] if exclude_self else [] for i in items]
    ix, sc = weighted_expect(_item_rows(B, items), inv, excl, n)
    q = np.broadcast_to(inv[np.asarray(items, np.int64)][:, None], sc.shape)
    real = np.isfinite(sc)                                  # (the padding stays -inf, also where the query's inv is 0)
    sc[real] = np.multiply(sc[real], q[real])
    assert sc.dtype == B.dtype
    return (ix, sc), n2


def test_similar_items(prec):
    """Session.similar_items and PoisMF.similar_items against the definition; self excluded or first; a zero row of B as a query (every
    similarity 0: index order) and as a candidate (similarity 0: last); item_norm= gives the same rows"""
    k, zrow = 50, 150
    A, B = _factors(DIMA, DIMB, k, prec, 58)
    B[zrow] = 0
    s = _session(DIMA, DIMB, k, prec, A, B)
    m = _model(A, B, k, prec)
    try:
        items = np.array([0, 7, zrow, 129, 130, 3076, 7] + list(range(1000, 1060)), np.uint64)   # 67 queries
        for n in (10, 128):
            for exclude_self in (True, False):
                want, n2 = _similar_expect(B, items, n, exclude_self)
                what = f"n {n} exclude_self {exclude_self}"
                same(s.similar_items(items, n, output_score=True, exclude_self=exclude_self), want, "session " + what)
                same(s.similar_items(items, n, output_score=True, exclude_self=exclude_self, item_norm=n2), want, "session, item_norm " + what)
                same(m.similar_items(items, n, output_score=True, exclude_self=exclude_self), want, "model " + what)
                same(m.similar_items(items, n, output_score=True, exclude_self=exclude_self, item_norm=n2), want, "model, item_norm " + what)
                others = np.flatnonzero(items != zrow)
                if exclude_self:
                    assert not (want[0] == items[:, None]).any()
                    assert want[0][2].tolist() == [j for j in range(n + 1) if j != zrow][:n]
                else:
                    assert np.array_equal(want[0][others, 0], items[others])      # the item itself leads: nothing is more similar
                    assert want[0][2].tolist() == list(range(n))
                assert not want[1][2].any() and not (want[0][others] == zrow).any()
        assert np.array_equal(s.item_norms(), n2)
        ix, sc = s.similar_items(items, 10)
        assert np.array_equal(ix, _similar_expect(B, items, 10, True)[0][0]) and sc.size == 0
    finally:
        s.close()

    # 40 items and n = 40: everything is listed, the zero row last among the real entries at similarity 0
    A, B = _factors(DIMA, 40, 7, prec, 12)
    B[11] = 0
    s = _session(DIMA, 40, 7, prec, A, B)
    try:
        items = np.arange(40, dtype=np.uint64)
        want, _ = _similar_expect(B, items, 40, True)
        got = s.similar_items(items, 40, output_score=True)
        same(got, want, "40 items")
        same(_model(A, B, 7, prec).similar_items(items, 40, output_score=True), want, "40 items, model")
        rest = np.flatnonzero(items != 11)
        assert np.all(got[0][rest, 38] == 11) and np.all(got[1][rest, 38] == 0) and np.all(got[0][:, 39] == api.TOPN_NONE)
    finally:
        s.close()


def test_the_session_is_left_as_it_was(prec):
    """topn_batch, topn_quota and topn_deep before and after a weighted call give the same rows (the calls share the session's
    scratch), and the factors are untouched"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 8)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        mod = (np.arange(DIMB) % 37).astype(np.uint64)
        w = _schemes(DIMB, H.dtype_of(prec), 4)["log-uniform"]
        others = lambda: (s.topn_batch(users, 10, exclude_seen=True, output_score=True),
                          s.topn_quota(users, 10, group_of=mod, quota=2, exclude_seen=True, output_score=True),
                          s.topn_deep(users, 300, exclude_seen=True, output_score=True))
        before = others()
        first = s.topn_weighted(users, 10, item_weight=w, exclude_seen=True, output_score=True)
        s.similar_items(users, 10)
        after = others()
        for b, a in zip(before, after):
            assert np.array_equal(b[0], a[0]) and b[1].tobytes() == a[1].tobytes()
        second = s.topn_weighted(users, 10, item_weight=w, exclude_seen=True, output_score=True)   # (after the deep call has grown the scratch)
        assert np.array_equal(first[0], second[0]) and first[1].tobytes() == second[1].tobytes()
        A2, B2 = s.get_factors()
        assert A2.tobytes() == A.tobytes() and B2.tobytes() == B.tobytes()
    finally:
        s.close()
