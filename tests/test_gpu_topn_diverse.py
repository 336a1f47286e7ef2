"""Diversified batched top-N (include/poismf_hip.h section 1p) on the GPU: picked items, relevance bits and value bits against the
definition rebuilt from the library's independent path, over k, both precisions and five (n, pool, lam) shapes; lam = 1 against the
deep and the plain call; short and empty rows; independence of the batch and of the item slices; the session against the host-pointer
entry; the return codes.

The expectation (diverse_expect; tests/test_topn_diverse_cpu.py holds it to hand-written answers): the user's whole score row from
predict_multiple(A, B) -- the pair_dot_kernel path, which the batched code does not share --, the pool by np.lexsort minus the
exclusions, the chains from predict_multiple(B, B, ., .), and the greedy loop in numpy in the model's precision, one elementwise
operation per rounding.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests import helpers as H

pytestmark = pytest.mark.gpu

DIMA, DIMB, BATCH = 90, 700, 150      # 150 batch entries: two tiles of 64 users and a part of a third
KS = (1, 7, 50, 130)                  # 130: a second 256-byte chunk of the gather in fp32 (the fifth in fp64)
SHAPES = ((10, 100, 0.7), (10, 10, 0.3), (128, 200, 0.5), (5, 65, 0.0), (3, 1024, 0.9))   # (n, pool, lam)
ZERO_ROWS = (213, 690)


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


# ---- the reference ----
def diverse_expect(rel_rows, chains, inv, excl, n, pool, lam):
    """Section 1p for every row of rel_rows [m x dimB] (the users' whole score rows, in the model's dtype): chains(P) gives the
    [c x c] fused chains among the rows of B of the items P, inv [dimB] the inverse norms, excl[i] row i's excluded items.  Every
    operation is one elementwise numpy operation in the rows' dtype.  Returns (items, relevances, values), [m x n] each, padded."""
    dt = rel_rows.dtype.type
    inv = np.asarray(inv)
    assert inv.dtype == rel_rows.dtype and inv.shape == (rel_rows.shape[1],)
    lam_t, oml = dt(lam), dt(1.0 - float(lam))
    m, dimB = rel_rows.shape
    ix = np.full((m, n), api.TOPN_NONE, np.uint64)
    sc = np.full((m, n), -np.inf, rel_rows.dtype)
    val = np.full((m, n), -np.inf, rel_rows.dtype)
    for i in range(m):
        idx = np.setdiff1d(np.arange(dimB), np.asarray(excl[i], np.int64))
        s = rel_rows[i, idx]
        P = idx[np.lexsort((idx, -s.astype(np.float64)))[:pool]]   # (the cast is exact; it only keeps -s in one dtype)
        c = len(P)
        if c == 0:
            continue
        rel = rel_rows[i, P]
        r = np.divide(rel, rel[0]) if rel[0] > 0 else rel
        lr = np.multiply(lam_t, r)
        G = chains(P)
        assert G.dtype == rel_rows.dtype and G.shape == (c, c) and lr.dtype == rel_rows.dtype
        mx = np.zeros(c, rel_rows.dtype)
        free = np.ones(c, bool)
        for t in range(min(n, c)):
            v = np.subtract(lr, np.multiply(oml, mx))
            cand = np.flatnonzero(free)
            q = cand[np.argmax(v[cand])]                            # (the first of equal values: the lowest position)
            ix[i, t], sc[i, t], val[i, t] = P[q], rel[q], v[q]
            free[q] = False
            cs = np.multiply(np.multiply(G[:, q], inv[P]), inv[P[q]])
            mx = np.where(cs > mx, cs, mx)
        assert val.dtype == rel_rows.dtype
    return ix, sc, val


def same(got, want, what):
    assert len(got) == 3 and all(g.shape == w.shape for g, w in zip(got, want)), what
    ok = np.array_equal(got[0], want[0]), got[1].tobytes() == want[1].tobytes(), got[2].tobytes() == want[2].tobytes()
    print(f"{what}: equal items {ok[0]} equal relevance bits {ok[1]} equal value bits {ok[2]}")
    if not ok[0]:
        bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
        raise AssertionError((what, "rows", bad[:8].tolist(), got[0][bad[0]][:12], want[0][bad[0]][:12]))
    assert ok[1] and ok[2], what


# ---- inputs ----
def make_factors(k, prec, seed=0, dimB=DIMB):
    """A [DIMA x k] and B [dimB x k]: rows 350 .. 449 of B repeat rows 0 .. 99 exactly (equal relevance and cosine 1: the tie rule),
    rows 450 .. 649 are rows 0 .. 199 with each entry moved by about one percent (near-duplicates), ZERO_ROWS are zero.  k = 1: every
    cosine among rows of one sign is 1, so only rows of another sign -- or zero -- can overtake: about 60 rows are positive, four of
    them large, the others negative, which puts the zero rows and the negative ones into a pool of 100."""
    rng = np.random.default_rng(1000 * k + seed)
    dt = H.dtype_of(prec)
    A = rng.random((DIMA, k)) ** 2 + 0.01
    if k == 1:
        B = -(0.001 + rng.random((dimB, 1)))
        pos = rng.choice(dimB, 60, replace=False)
        B[pos[:4], 0] = 0.8 + 0.2 * rng.random(4)
        B[pos[4:], 0] = 0.05 + 0.25 * rng.random(56)
    else:
        B = 2.0 * rng.random((dimB, k)) ** 4 + 2.0 ** -10
    B[350:450] = B[0:100]
    B[450:650] = B[0:200] * (1.0 + 0.01 * rng.standard_normal((200, k)))
    B[list(ZERO_ROWS)] = 0
    return np.ascontiguousarray(A, dtype=dt), np.ascontiguousarray(B, dtype=dt)


def batch_users(seed=0):
    """150 batch entries over 90 users: unordered, with repeats"""
    return np.random.default_rng(seed).integers(0, DIMA, BATCH).astype(np.uint64)


def score_rows(A, B, users):
    """the users' whole score rows from predict_multiple: [len(users) x dimB]"""
    users = np.asarray(users, np.uint64)
    dimB = B.shape[0]
    out = np.empty(len(users) * dimB, B.dtype)
    api._predict_multiple(out, A, B, np.repeat(users, dimB), np.tile(np.arange(dimB, dtype=np.uint64), len(users)))
    return out.reshape(len(users), dimB)


def chain_block(B, P):
    """predict_multiple(B, B, ., .) for every pair of the items P: [c x c]"""
    P = np.asarray(P, np.uint64)
    out = np.empty(len(P) * len(P), B.dtype)
    if len(P):
        api._predict_multiple(out, B, B, np.repeat(P, len(P)), np.tile(P, len(P)))
    return out.reshape(len(P), len(P))


def norms(B):
    """(the squared norms predict_multiple gives, their inverse roots as section 1p wants them)"""
    every = np.arange(B.shape[0], dtype=np.uint64)
    n2 = np.empty(B.shape[0], B.dtype)
    api._predict_multiple(n2, B, B, every, every)
    inv = np.zeros(B.shape[0], B.dtype)
    nz = n2 != 0
    inv[nz] = B.dtype.type(1) / np.sqrt(n2[nz])
    assert inv.dtype == B.dtype
    return n2, inv


def model_of(A, B, prec):
    m = api.PoisMF(k=A.shape[1], use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, A.shape[0], B.shape[0], True
    return m


def excl_pair(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


def near_the_top(A, B, users, step, depth):
    """per batch entry, every step-th of its best `depth` items by a host product (which items exactly does not matter): sorted lists"""
    approx = A[users.astype(np.int64)].astype(np.float64) @ B.astype(np.float64).T
    best = np.argsort(-approx, axis=1, kind="stable")[:, :depth:step]
    return [np.sort(r) for r in best]


_SETUP = {}


def setup_of(k, prec):
    """(A, B, users, score rows, the chains among all items, squared norms, inverse norms), computed once per (k, precision)"""
    if (k, prec) not in _SETUP:
        A, B = make_factors(k, prec)
        users = batch_users()
        n2, inv = norms(B)
        G = chain_block(B, np.arange(DIMB))
        for a in (G, inv, n2):
            a.setflags(write=False)
        _SETUP[k, prec] = A, B, users, score_rows(A, B, users), G, n2, inv
    return _SETUP[k, prec]


# ---- 1. the definition ----
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-pool%d-lam%g" % s)
@pytest.mark.parametrize("k", KS)
def test_bits_against_the_definition(prec, k, shape):
    n, pool, lam = shape
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    assert np.array_equal(B[350:450], B[0:100]) and not B[list(ZERO_ROWS)].any() and inv[ZERO_ROWS[0]] == 0
    excl = near_the_top(A, B, users, 3, 30)
    model = model_of(A, B, prec)
    chains = lambda P: G[np.ix_(P, P)]
    for how, e in (("plain", [np.empty(0, np.int64)] * BATCH), ("excluded", excl)):
        want = diverse_expect(rows, chains, inv, e, n, pool, lam)
        got = model.topN_diverse(users, n, pool, lam, exclude=None if how == "plain" else excl_pair(e), output_score=True, output_value=True)
        same(got, want, f"k {k} n {n} pool {pool} lam {lam} {how}")
        if how == "plain" and lam == 0.7:
            plain = model.topN_batch(users, n)[0]
            differ = int((want[0] != plain).any(axis=1).sum())
            print(f"k {k}: MMR changes the top {n} of {differ} of {BATCH} rows")
            assert 10 * differ >= BATCH      # (a condition on the inputs: a kernel that ignores the cosines cannot pass)
    ix, sc, val = model.topN_diverse(users, n, pool, lam, exclude=excl_pair(excl))   # (neither optional output asked for)
    assert np.array_equal(ix, want[0]) and sc.size == 0 and val.size == 0


def test_exact_duplicates_meet_the_tie_rule(prec):
    """the inputs do exercise the tie rule: in some pool an item and its exact copy stand next to each other with equal relevance"""
    A, B, users, rows, G, n2, inv = setup_of(50, prec)
    assert np.array_equal(rows[:, 350:450], rows[:, 0:100])
    assert np.array_equal(G[350:450, 350:450], G[0:100, 0:100])
    deep = model_of(A, B, prec).topN_deep(users, 100)[0].astype(np.int64)
    met = int(((deep[:, 1:] - deep[:, :-1] == 350) & (deep[:, :-1] < 100)).sum())
    print(f"twins next to each other in a pool of 100: {met}")
    assert met > BATCH


# ---- 2. lam = 1 ----
@pytest.mark.parametrize("k", (7, 50))
def test_lam_one_is_the_plain_list(prec, k):
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    model = model_of(A, B, prec)
    excl = excl_pair(near_the_top(A, B, users, 2, 40))
    for n, pool in ((1, 1), (10, 100), (10, 10), (128, 128), (128, 1024)):
        for e in (None, excl):
            ix, sc, val = model.topN_diverse(users, n, pool, 1.0, exclude=e, output_score=True, output_value=True)
            for other in (model.topN_deep(users, n, exclude=e, output_score=True), model.topN_batch(users, n, exclude=e, output_score=True)):
                assert np.array_equal(ix, other[0]) and sc.tobytes() == other[1].tobytes(), (n, pool)
            assert np.all(val[:, 0] == 1) and np.all(np.diff(val.astype(np.float64), axis=1) <= 0)   # v = rel / rel_0


# ---- 3. short rows ----
def test_short_and_empty_rows_are_padded(prec):
    """exclusions that leave 0, 1, n - 1 and pool - 1 admissible items, beside users that keep everything"""
    k, n, pool, lam = 50, 10, 100, 0.7
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    users = users[:70]
    rng = np.random.default_rng(5)
    everything = np.arange(DIMB)
    excl = [np.empty(0, np.int64)] * len(users)
    left = {3: 0, 17: 1, 40: n - 1, 69: pool - 1}
    for row, keep in left.items():
        excl[row] = np.setdiff1d(everything, rng.choice(DIMB, keep, replace=False))
    want = diverse_expect(rows[:70], lambda P: G[np.ix_(P, P)], inv, excl, n, pool, lam)
    model = model_of(A, B, prec)
    got = model.topN_diverse(users, n, pool, lam, exclude=excl_pair(excl), output_score=True, output_value=True)
    same(got, want, "short rows")
    for row, keep in left.items():
        c = min(keep, n)
        assert np.all(got[0][row, :c] != api.TOPN_NONE) and np.all(np.isfinite(got[1][row, :c])) and np.all(np.isfinite(got[2][row, :c]))
        assert np.all(got[0][row, c:] == api.TOPN_NONE) and np.all(got[1][row, c:] == -np.inf) and np.all(got[2][row, c:] == -np.inf)
    few = np.array([3, 17], np.int64)                    # (two users: many item slices and the merge)
    got2 = model.topN_diverse(users[few], n, pool, lam, exclude=excl_pair([excl[3], excl[17]]), output_score=True, output_value=True)
    same(got2, tuple(w[few] for w in want), "short rows, two users")


# ---- 4. independence ----
def test_a_row_does_not_depend_on_the_batch(prec):
    k, n, pool, lam = 50, 10, 100, 0.7
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    s = session_of(A, B, prec)
    try:
        call = lambda u: s.topn_diverse(u, n, pool, lam, output_score=True, output_value=True, item_norm=n2)
        whole = call(users)
        same(whole, diverse_expect(rows, lambda P: G[np.ix_(P, P)], inv, [[]] * BATCH, n, pool, lam), "the batch of 150")
        for u in np.unique(users):
            alone = call([u])
            for p in np.flatnonzero(users == u):
                assert all(a[0].tobytes() == w[p].tobytes() for a, w in zip(alone, whole)), int(u)
    finally:
        s.close()


def test_item_slices_do_not_change_a_row(prec):
    """20 011 items at k = 8 and five users: the deep stage cuts the items into slices and merges them"""
    k, dimB, n, pool, lam = 8, 20011, 10, 100, 0.7
    A, B = make_factors(k, prec, seed=3, dimB=dimB)
    users = np.array([5, 80, 5, 0, 33], np.uint64)
    n2, inv = norms(B)
    want = diverse_expect(score_rows(A, B, users), lambda P: chain_block(B, P), inv, [[]] * len(users), n, pool, lam)
    got = model_of(A, B, prec).topN_diverse(users, n, pool, lam, output_score=True, output_value=True)
    same(got, want, "20 011 items")
    assert got[0][0].tobytes() == got[0][2].tobytes()


# ---- 5. the session ----
def session_of(A, B, prec, seen_rows=None):
    dimA, dimB = A.shape[0], B.shape[0]
    if seen_rows is None:
        seen_rows = [np.array([i % dimB]) for i in range(dimA)]
    row = np.concatenate([np.full(len(r), i) for i, r in enumerate(seen_rows)])
    s = api.Session.from_coo(sp.coo_matrix((np.ones(len(row)), (row, np.concatenate(seen_rows))), shape=(dimA, dimB)), A.shape[1], prec)
    s.set_factors(A, B)
    return s


@pytest.mark.parametrize("k", (7, 130))
def test_session_equals_the_host_pointer_call(prec, k):
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    everyone = np.arange(DIMA, dtype=np.uint64)
    seen = near_the_top(A, B, everyone, 2, 60)
    extra = near_the_top(A, B, users, 3, 90)
    s = session_of(A, B, prec, seen)
    model = model_of(A, B, prec)
    try:
        assert np.array_equal(s.item_norms(), n2)
        for n, pool, lam in ((10, 100, 0.7), (128, 200, 0.5)):
            kw = dict(output_score=True, output_value=True)
            host_seen = model.topN_diverse(users, n, pool, lam, exclude=excl_pair([seen[int(u)] for u in users]), **kw)
            same(s.topn_diverse(users, n, pool, lam, exclude_seen=True, **kw), host_seen, f"exclude_seen n {n}")
            same(s.topn_diverse(users, n, pool, lam, exclude_seen=True, item_norm=s.item_norms(), **kw), host_seen, f"exclude_seen, item_norm n {n}")
            host_list = model.topN_diverse(users, n, pool, lam, exclude=excl_pair(extra), **kw)
            same(s.topn_diverse(users, n, pool, lam, exclude=excl_pair(extra), **kw), host_list, f"exclude= n {n}")
            same(model.topN_diverse(users, n, pool, lam, exclude=excl_pair(extra), item_norm=n2, **kw), host_list, f"model, item_norm n {n}")
            both = [np.union1d(seen[int(u)], e) for u, e in zip(users, extra)]
            same(s.topn_diverse(users, n, pool, lam, exclude_seen=True, exclude=excl_pair(extra), **kw),
                 model.topN_diverse(users, n, pool, lam, exclude=excl_pair(both), **kw), f"both n {n}")
        before = s.topn_deep(users, 300, output_score=True)
        s.topn_diverse(users, 10, 100, 0.7)
        after = s.topn_deep(users, 300, output_score=True)          # (the calls share the session's scratch)
        assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()
        A2, B2 = s.get_factors()
        assert A2.tobytes() == A.tobytes() and B2.tobytes() == B.tobytes()
    finally:
        s.close()


def test_r_flavour(prec):
    if prec:
        return   # (the R flavour is double)
    A, B, users, rows, G, n2, inv = setup_of(50, prec)
    n, pool, lam = 10, 100, 0.7
    want = model_of(A, B, prec).topN_diverse(users, n, pool, lam, output_score=True, output_value=True)
    lib = api.load_library("r")
    u = np.ascontiguousarray(users.astype(np.int32))
    out, sc, val = np.zeros((BATCH, n), np.int32), np.zeros((BATCH, n), np.float64), np.zeros((BATCH, n), np.float64)
    p = api._ptr
    assert lib.poismf_hip_topn_diverse(p(A), p(B), 50, DIMA, DIMB, p(u), BATCH, n, pool, lam, p(inv), None, None, p(out), p(sc), p(val)) == 0
    assert np.array_equal(out.astype(np.int64).astype(np.uint64), want[0]) and sc.tobytes() == want[1].tobytes() and val.tobytes() == want[2].tobytes()


# ---- 6. return codes ----
def test_return_code_2_leaves_the_outputs_untouched(prec):
    k = 7
    A, B, users, rows, G, n2, inv = setup_of(k, prec)
    dt = H.dtype_of(prec)
    s = session_of(A, B, prec)
    lib = api.load_library(prec)
    p = api._ptr
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    ok = dict(users=u64([0, 1]), n=5, pool=20, lam=0.5, inv=inv, excl=None)
    bad_inv = lambda j, x: np.concatenate([inv[:j], np.array([x], dt), inv[j + 1:]])
    cases = {
        "n-zero": dict(n=0), "n-above-128": dict(n=129, pool=200), "pool-below-n": dict(pool=4), "pool-above-1024": dict(pool=1025),
        "lam-nan": dict(lam=float("nan")), "lam-negative": dict(lam=-1e-9), "lam-above-one": dict(lam=1.0000001),
        "inv-null": dict(inv=None), "inv-nan": dict(inv=bad_inv(3, np.nan)), "inv-inf": dict(inv=bad_inv(0, np.inf)),
        "inv-negative": dict(inv=bad_inv(DIMB - 1, -1e-30)), "user-out-of-range": dict(users=u64([0, DIMA])),
        "item-out-of-range": dict(excl=(u64([0, 1, 2]), u64([3, DIMB]))), "descending-row": dict(excl=(u64([0, 2, 4]), u64([1, 2, 9, 7]))),
    }
    try:
        for name, change in cases.items():
            c = {**ok, **change}
            for entry in ("host", "session"):
                out = np.full((2, max(c["n"], 1)), 12345, np.uint64)
                sc, val = np.full(out.shape, -7.0, dt), np.full(out.shape, -7.0, dt)
                ep, ei = c["excl"] if c["excl"] is not None else (None, None)
                tail = (p(c["inv"]) if c["inv"] is not None else None,)
                outs = (p(ep) if ep is not None else None, p(ei) if ei is not None else None, p(out), p(sc), p(val))
                if entry == "host":
                    rc = lib.poismf_hip_topn_diverse(p(A), p(B), k, DIMA, DIMB, p(c["users"]), 2, c["n"], c["pool"], c["lam"], *tail, *outs)
                else:
                    rc = lib.poismf_hip_session_topn_diverse(s.h, p(c["users"]), 2, c["n"], c["pool"], c["lam"], *tail, 0, *outs)
                assert rc == 2, (name, entry)
                assert np.all(out == 12345) and np.all(sc == -7.0) and np.all(val == -7.0), (name, entry)
        out = np.full((2, 5), 12345, np.uint64)
        assert lib.poismf_hip_session_topn_diverse(s.h, p(ok["users"]), 0, 5, 20, 0.5, None, 0, None, None, p(out), None, None) == 0
        assert lib.poismf_hip_session_topn_diverse(s.h, p(ok["users"]), 2, 5, 20, 0.5, p(inv), 0, None, None, p(out), None, None) == 0
        assert np.all(out != 12345)
        for bad in (dict(top_n=0), dict(top_n=129, pool=200), dict(pool=4), dict(pool=1025), dict(lam=float("nan")), dict(lam=1.5)):
            with pytest.raises(ValueError):
                s.topn_diverse([0, 1], **{**dict(top_n=5, pool=20, lam=0.5), **bad})
    finally:
        s.close()
