"""Fold-in of new users on a resident session (include/poismf_hip.h section 1m) on the GPU: the factors bit for bit those of
factors_multiple and within the parity bounds of the oracle; top-N and ranks straight off those factors against the lexsort of the
pair-dot path's whole score row; a host session that is left exactly as it was; the host-pointer drop-in; and what the session
entries refuse on a live session.

Shapes: a session of 600 x 6000; 130 new rows (two full 64-user tiles and a tile of two) of 0, 1, 15, 16, 17, ~40 and 300
nonzeros; in the top-N and rank tests one row of 4500, past the 4096 at which exclusion staging changes.  One world per
(precision, k) is built once and shared; nothing in it is written after it is built."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bindings
from poismf_amd import api, harness, metrics
from tests import helpers as H

pytestmark = pytest.mark.gpu

DIMA, DIMB, NNEW = 600, 6000, 130
LENGTHS = {0: 0, 1: 1, 2: 15, 3: 16, 4: 17, 5: 300, 63: 0, 64: 1, 129: 17}   # the other rows: 30 .. 50
LONG_ROW, LONG_LEN = 70, 4500
KS = [5, 50, 65]
NITER = 3


def T(is_float, t64, t32):
    return t32 if is_float else t64


def _ids(prec, k):
    return f"{'f32' if prec else 'f64'}-k{k}"


WORLDS = [(p, k) for p in (False, True) for k in KS]
WORLD_IDS = [_ids(p, k) for p, k in WORLDS]


@functools.lru_cache(maxsize=None)
def _known_items():
    """the items somebody in the resident model's matrix has (its pattern is the same for every k and precision): an item nobody
    has gets an all-zero row of B, and a new row that names it has no finite objective, in the reference either"""
    _, csc, _, _ = H.small_problem(DIMA, DIMB, 24000, 5, False, seed=21)
    return np.flatnonzero(np.diff(csc[2].astype(np.int64)))


def _new_rows(long_row, seed=5):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(NNEW):
        n = LENGTHS.get(r, int(rng.integers(30, 51)))
        if long_row and r == LONG_ROW:
            n = LONG_LEN
        rows.append(np.full(n, r))
        cols.append(np.sort(rng.choice(_known_items(), n, replace=False)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    val = 1.0 + np.floor(rng.gamma(1.0, 1.0, len(rows)))
    X = sp.csr_matrix((val, (rows, cols)), shape=(NNEW, DIMB))
    X.sum_duplicates(); X.sort_indices()
    return X


class World:
    """a resident model (600 x 6000 after one CG sweep), its statistics, and the new rows"""

    def __init__(self, prec, k):
        self.prec, self.k, self.dt = prec, k, H.dtype_of(prec)
        csr, csc, A0, B0 = H.small_problem(DIMA, DIMB, 24000, k, prec, seed=21)
        self.sess = api.Session(csr, csc, DIMA, DIMB, k, prec)
        self.sess.set_factors(A0, B0)
        l2, maxupd, _ = harness.auto_defaults("cg", k)
        self.sess.sweep(self.sess.make_params("cg", l2, maxupd=maxupd), 1e-7)
        self.A, self.B = self.sess.get_factors()
        self.Bsum = self.B.sum(axis=0).astype(self.dt)
        self.Amean = self.A.mean(axis=0).astype(self.dt)
        self.X = _new_rows(False)
        self.Xlong = _new_rows(True)
        self.csr = (csr, csc)

    def params(self, method, w=1.0, reuse=False):
        l2, maxupd, _ = harness.auto_defaults(method, self.k)
        return self.sess.make_params(method, l2, 0.0, w, 1e-7, True, maxupd, False, reuse), l2, maxupd

    def stats(self):
        return dict(Bsum=self.Bsum, Amean=self.Amean)

    @functools.lru_cache(maxsize=None)
    def served(self):
        """the CG factors of Xlong and their whole score rows from the pair-dot path (predict_multiple): computed once"""
        p, _, _ = self.params("cg")
        A_new = self.sess.transform(self.Xlong, p, NITER, **self.stats())
        out = np.empty(NNEW * DIMB, self.dt)
        api._predict_multiple(out, A_new, self.B, np.repeat(np.arange(NNEW, dtype=np.uint64), DIMB),
                              np.tile(np.arange(DIMB, dtype=np.uint64), NNEW))
        out = out.reshape(NNEW, DIMB)
        A_new.setflags(write=False); out.setflags(write=False)
        return p, A_new, out


_worlds = {}


def world(prec, k):
    if (prec, k) not in _worlds:
        _worlds[(prec, k)] = World(prec, k)
    return _worlds[(prec, k)]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _worlds.values():
        w.sess.close()
    _worlds.clear()


def _u(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _rows(X):
    return [X.indices[X.indptr[r]:X.indptr[r + 1]].astype(np.int64) for r in range(X.shape[0])]


def _pair(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


def _order(score_row, excluded):
    """the admissible items under (score descending, item ascending), and their scores"""
    idx = np.setdiff1d(np.arange(len(score_row)), np.asarray(excluded, np.int64))
    sc = score_row[idx]
    o = np.lexsort((idx, -sc.astype(np.float64)))   # (the cast is exact; it only keeps -sc in one dtype)
    return idx[o], sc[o]


def _extra(seed=9):
    """an extra exclusion list per new row: 25 items, ten of them the row's own where it has that many"""
    rng = np.random.default_rng(seed)
    own = _rows(_new_rows(True))
    return [np.unique(np.concatenate((rng.choice(DIMB, 15, replace=False), own[r][:10]))) for r in range(NNEW)]


# ---- 1. factors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,k", WORLDS, ids=WORLD_IDS)
@pytest.mark.parametrize("method", ["pg", "cg", "tncg"])
@pytest.mark.parametrize("w", [1.0, 3.0])
@pytest.mark.parametrize("reuse", [True, False])
def test_transform_is_factors_multiple(prec, k, method, w, reuse):
    """array_equal to factors_multiple on the same B, Bsum, Amean and rows; the oracle's factors_multiple at the parity bounds"""
    W = world(prec, k)
    p, l2, maxupd = W.params(method, w, reuse)
    X = W.X
    A1 = W.sess.transform(X, p, NITER, **W.stats())
    data, indptr, indices = X.data.astype(W.dt), _u(X.indptr), _u(X.indices)
    A2 = api._predict_factors_multiple(W.B, W.Bsum, W.Amean, indptr, indices, data, l2, w, 1e-7, NITER, maxupd, method, True, reuse, 1)
    assert A1.shape == (NNEW, k) and A1.dtype == W.dt
    assert np.array_equal(A1, A2)
    empty = np.diff(X.indptr) == 0
    assert empty.sum() == 2 and not A1[empty].any() and A1.any() and np.isfinite(A1).all()
    Ao = bindings.Oracle(prec).factors_multiple(W.B, W.Bsum, W.Amean, data, indptr, indices, l2, w, 1e-7, NITER, maxupd, method, True, reuse)
    if method == "pg":
        err = H.scaled_err(A1, Ao)
        print(f"pg scaled_err {err:.3e}")
        assert err <= T(prec, 1e-12, 1e-5)
    else:
        l2o = l2 if method == "cg" else 0.0
        fo = H.half_objective(A1, W.B, data, indices, indptr, W.Bsum, l2o, w)
        fr = H.half_objective(Ao, W.B, data, indices, indptr, W.Bsum, l2o, w)
        print(f"{method} objective rel {abs(fo - fr) / abs(fr):.3e}")
        assert abs(fo - fr) <= T(prec, 1e-6, 2e-2) * abs(fr)


@pytest.mark.parametrize("prec,k", [(False, 5), (True, 50)], ids=[_ids(False, 5), _ids(True, 50)])
def test_transform_defaults_and_empty_batches(prec, k):
    """the statistics default to those of PoisMF.fit for the resident factors; an all-empty batch gives zeros; so does no row"""
    W = world(prec, k)
    p, _, _ = W.params("cg")
    assert np.array_equal(W.sess.transform(W.X, p, NITER), W.sess.transform(W.X, p, NITER, **W.stats()))
    Z = W.sess.transform(sp.csr_matrix((7, DIMB)), p, NITER, **W.stats())
    assert Z.shape == (7, k) and not Z.any()
    ix, sc, Z = W.sess.topn_new(sp.csr_matrix((7, DIMB)), p, NITER, top_n=4, output_score=True, return_factors=True, **W.stats())
    assert not Z.any() and not sc.any() and np.array_equal(ix, np.tile(np.arange(4, dtype=np.uint64), (7, 1)))
    assert W.sess.transform(sp.csr_matrix((0, DIMB)), p, NITER, **W.stats()).shape == (0, k)
    # the guest is refilled, not remembered: the rows again, after a smaller and an empty batch
    full = W.sess.transform(W.X, p, NITER, **W.stats())
    assert np.array_equal(W.sess.transform(W.X[:70], p, NITER, **W.stats()), full[:70])
    assert np.array_equal(W.sess.transform(W.X, p, NITER, **W.stats()), full)


# ---- 2. top-N ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,k", WORLDS, ids=WORLD_IDS)
@pytest.mark.parametrize("own", [True, False], ids=["own", "all"])
@pytest.mark.parametrize("extra", [False, True], ids=["", "extra"])
def test_topn_new_against_the_pair_dot_path(prec, k, own, extra):
    W = world(prec, k)
    p, A_new, scores = W.served()
    rows, more = _rows(W.Xlong), _extra()
    for n in (1, 10, 128):
        ix, sc, fac = W.sess.topn_new(W.Xlong, p, NITER, top_n=n, exclude_own=own, exclude=_pair(more) if extra else None, output_score=True,
                                      return_factors=True, **W.stats())
        assert np.array_equal(fac, A_new)
        assert ix.shape == (NNEW, n) and sc.shape == (NNEW, n)
        for r in range(NNEW):
            excl = np.concatenate((rows[r] if own else np.empty(0, np.int64), more[r] if extra else np.empty(0, np.int64)))
            eix, esc = _order(scores[r], excl)
            assert np.array_equal(ix[r], eix[:n].astype(np.uint64)), (r, n)
            assert np.array_equal(sc[r], esc[:n]), (r, n)
    if own and not extra:
        assert not A_new[0].any() and np.array_equal(ix[0], np.arange(128, dtype=np.uint64))   # the zero-factor row: items by index
        assert not np.isin(ix[LONG_ROW], rows[LONG_ROW]).any()                                  # the 4500-item row is excluded
    if not own and not extra:
        ix2, sc2 = W.sess.topn_new(W.Xlong, p, NITER, top_n=10, exclude_own=False, **W.stats())
        assert sc2.shape == (0, 10) and np.array_equal(ix2, ix[:, :10])


@pytest.mark.parametrize("prec,k", [(False, 50), (True, 50), (True, 65)], ids=[_ids(False, 50), _ids(True, 50), _ids(True, 65)])
def test_topn_new_rows_alone_and_too_few_left(prec, k):
    W = world(prec, k)
    p, A_new, scores = W.served()
    ix, sc = W.sess.topn_new(W.Xlong, p, NITER, top_n=10, output_score=True, **W.stats())
    for r in (0, 63, 64, LONG_ROW, 129):
        ix1, sc1, f1 = W.sess.topn_new(W.Xlong[r], p, NITER, top_n=10, output_score=True, return_factors=True, **W.stats())
        assert np.array_equal(f1[0], A_new[r]) and np.array_equal(ix1[0], ix[r]) and np.array_equal(sc1[0], sc[r])
    # the long row's 4500 items and 1495 others leave 5: fewer than 10, and only the union shows it
    rest = np.setdiff1d(np.arange(DIMB), _rows(W.Xlong)[LONG_ROW])[:1495]
    excl = [np.empty(0, np.int64)] * NNEW
    excl[LONG_ROW] = rest
    with pytest.raises(ValueError):
        W.sess.topn_new(W.Xlong, p, NITER, top_n=10, exclude=_pair(excl), **W.stats())
    ix5, _ = W.sess.topn_new(W.Xlong, p, NITER, top_n=5, exclude=_pair(excl), **W.stats())
    assert np.array_equal(ix5[LONG_ROW], _order(scores[LONG_ROW], np.concatenate((rest, _rows(W.Xlong)[LONG_ROW])))[0][:5].astype(np.uint64))


# ---- 3. ranks ---------------------------------------------------------------------------------------------------------------
def _held_out(seed=13):
    """per new row 6 held-out items: three of its own (where it has them), three others"""
    rng = np.random.default_rng(seed)
    own = _rows(_new_rows(True))
    return [np.unique(np.concatenate((own[r][:3], rng.choice(DIMB, 3, replace=False)))) for r in range(NNEW)]


@pytest.mark.parametrize("prec,k", WORLDS, ids=WORLD_IDS)
@pytest.mark.parametrize("own", [True, False], ids=["own", "all"])
def test_rank_new_against_the_pair_dot_path(prec, k, own):
    W = world(prec, k)
    p, A_new, scores = W.served()
    rows, more, test = _rows(W.Xlong), _extra(), _held_out()
    tp, ti = _pair(test)
    ranks, n_adm, fac = W.sess.rank_new(W.Xlong, (tp, ti), p, NITER, exclude_own=own, exclude=_pair(more), return_factors=True, **W.stats())
    assert np.array_equal(fac, A_new)
    ix, _ = W.sess.topn_new(W.Xlong, p, NITER, top_n=128, exclude_own=own, exclude=_pair(more), **W.stats())
    for r in range(NNEW):
        excl = np.unique(np.concatenate((rows[r] if own else np.empty(0, np.int64), more[r])))
        order, _ = _order(scores[r], excl)
        assert n_adm[r] == DIMB - len(excl)
        pos = {int(j): i for i, j in enumerate(order)}
        for c, t in enumerate(test[r]):
            got = int(ranks[int(tp[r]) + c])
            if int(t) in excl:
                assert got == api.RANK_EXCLUDED
            else:
                assert got == pos[int(t)], (r, int(t))
                if got < 128:
                    assert int(ix[r, got]) == int(t)
    if own:
        assert (ranks == api.RANK_EXCLUDED).sum() >= 3 * (NNEW - 10)   # every own item is excluded


@pytest.mark.parametrize("prec,k", [(False, 50), (True, 50)], ids=[_ids(False, 50), _ids(True, 50)])
def test_eval_ranking_new_is_metrics_of_those_ranks(prec, k):
    W = world(prec, k)
    p, _, _ = W.served()
    test = _held_out(17)
    tp, ti = _pair(test)
    Xt = sp.csr_matrix((np.ones(len(ti)), ti.astype(np.int64), tp.astype(np.int64)), shape=(NNEW, DIMB))
    ranks, n_adm = W.sess.rank_new(W.Xlong, (tp, ti), p, NITER, **W.stats())
    got = W.sess.eval_ranking_new(W.Xlong, Xt, p, NITER, k=10, per_user=True, **W.stats())
    assert np.array_equal(got["ranks"], ranks) and np.array_equal(got["n_adm"], n_adm)
    each = metrics.metrics_from_ranks(tp, ranks, n_adm, 10)
    want = metrics.mean_metrics(each)
    for name, v in want.items():
        np.testing.assert_equal(got[name], v, err_msg=name)
    assert want["n_users"] > 0


# ---- 4. the host session is untouched -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,k,method", [(True, 50, "pg"), (False, 50, "cg")], ids=["pg-f32-k50", "cg-f64-k50"])
def test_the_host_session_is_untouched(prec, k, method):
    """sweep, the three fold-in calls, sweep == sweep, sweep; factors and exclude_seen answers the same before and after a fold-in"""
    csr, csc, A0, B0 = H.small_problem(DIMA, DIMB, 24000, k, prec, seed=21)
    l2, maxupd, _ = harness.auto_defaults(method, k)
    X, test = _new_rows(True), _pair(_held_out())
    users = np.arange(0, DIMA, 7, dtype=np.uint64)
    dt = H.dtype_of(prec)
    Bsum, Amean = B0.sum(axis=0).astype(dt), A0.mean(axis=0).astype(dt)
    out = []
    for fold in (True, False):
        s = api.Session(csr, csc, DIMA, DIMB, k, prec)
        try:
            s.set_factors(A0, B0)
            p = s.make_params(method, l2, maxupd=maxupd)
            if fold:   # (before any sweep the padded copy of B is stale: the fold-in refreshes it for the session)
                s.transform(X, p, NITER, Bsum=Bsum, Amean=Amean)
            step = s.sweep(p, 1e-7)
            if fold:
                A1, B1 = s.get_factors()
                seen = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
                s.transform(X, p, NITER, Bsum=Bsum, Amean=Amean)
                s.topn_new(X, p, NITER, Bsum=Bsum, Amean=Amean)
                s.rank_new(X, test, p, NITER, Bsum=Bsum, Amean=Amean)
                A2, B2 = s.get_factors()
                assert np.array_equal(A1, A2) and np.array_equal(B1, B2)
                again = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
                assert np.array_equal(seen[0], again[0]) and np.array_equal(seen[1], again[1])
            s.sweep(p, step)
            out.append(s.get_factors())
        finally:
            s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 5. the drop-in -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["pg", "cg"])
def test_poismf_topn_new_is_transform_then_topn(prec, method):
    W = world(prec, 50)
    m = api.PoisMF(k=50, method=method, use_float=prec, niter=NITER)
    m.A, m.B, m.nusers, m.nitems = W.A, W.B, DIMA, DIMB
    m.Bsum, m.Amean = W.B.sum(axis=0), W.A.mean(axis=0)
    m.is_fitted = True
    X = W.Xlong
    fac = m.transform(X)
    holder = api.PoisMF(k=50, use_float=prec)
    holder.A, holder.B, holder.nusers, holder.nitems, holder.is_fitted = fac, W.B, NNEW, DIMB, True
    want = holder.topN_batch(np.arange(NNEW), 10, exclude=X, output_score=True)
    got = m.topN_new(X, 10, output_score=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one = m.topN_new(X[64], 10, output_score=True)
    assert np.array_equal(one[0][0], want[0][64]) and np.array_equal(one[1][0], want[1][64])
    everything = m.topN_new(X, 10, exclude_own=False)
    assert np.array_equal(everything[0], holder.topN_batch(np.arange(NNEW), 10)[0]) and everything[1].shape == (0, 10)


@pytest.mark.parametrize("prec", [False, True], ids=["f64", "f32"])
def test_exclude_own_with_rows_in_the_caller_s_order(prec):
    """a C caller's rows need not ascend and may name an item twice (the Python layer sorts and merges): exclude_own then scans the
    rows, as exclude_seen scans such resident rows, and the answer is still the lexsort of the returned factors' score rows"""
    W = world(prec, 50)
    par, _, _ = W.params("cg")
    items = _known_items()
    own = [items[[40, 7, 40, 300, 12]], items[[5]], items[np.arange(90, 20, -1)]]
    ip, ii = _pair(own)
    X = np.ones(len(ii), W.dt)
    n = 10
    ix, sc, fac = np.empty((3, n), np.uint64), np.empty((3, n), W.dt), np.empty((3, 50), W.dt)
    p = api._ptr
    rc = W.sess.lib.poismf_hip_session_topn_new(W.sess.h, p(X), p(ip), p(ii), 3, p(W.Bsum), p(W.Amean), C.byref(par), NITER, n, 1, None, None,
                                                p(ix), p(sc), p(fac))
    assert rc == 0 and fac.any(axis=1).all()
    scores = np.empty(3 * DIMB, W.dt)
    api._predict_multiple(scores, fac, W.B, np.repeat(np.arange(3, dtype=np.uint64), DIMB), np.tile(np.arange(DIMB, dtype=np.uint64), 3))
    scores = scores.reshape(3, DIMB)
    tp, ti = _pair([np.sort(np.unique(r))[:2] for r in own])
    rk, na = np.empty(len(ti), np.uint32), np.empty(3, np.uint32)
    rc = W.sess.lib.poismf_hip_session_rank_new(W.sess.h, p(X), p(ip), p(ii), 3, p(W.Bsum), p(W.Amean), C.byref(par), NITER, p(tp), p(ti), 1,
                                                None, None, p(rk), p(na), None)
    assert rc == 0 and np.all(rk == api.RANK_EXCLUDED)
    for r in range(3):
        eix, esc = _order(scores[r], own[r])
        assert np.array_equal(ix[r], eix[:n].astype(np.uint64)) and np.array_equal(sc[r], esc[:n])
        assert na[r] == DIMB - len(np.unique(own[r]))


# ---- what the session entries refuse on a live session ------------------------------------------------------------------------
def test_session_entries_return_2_and_write_nothing():
    W = world(True, 5)
    lib, dt = W.sess.lib, np.float32
    par, _, _ = W.params("pg")
    p = api._ptr
    X = np.ones(3, dt)
    held_p, held_i = _u([0, 2, 3]), _u([4, 9, 7])
    out, sc, fac = np.full((2, 5), 12345, np.uint64), np.full((2, 5), -7.0, dt), np.full((2, 5), -7.0, dt)
    rk, na = np.full(3, 12345, np.uint32), np.full(2, 12345, np.uint32)
    # rows that are no CSR of this model's items
    for indptr, indices in (([0, 2, 3], [4, DIMB, 7]), ([0, 2, 3], [4, -3, 7]), ([0, 2, 1], [4, 9, 7]), ([-1, 2, 3], [4, 9, 7])):
        ip, ii = np.asarray(indptr, np.int64).view(np.uint64).copy(), np.asarray(indices, np.int64).view(np.uint64).copy()
        lead = [W.sess.h, p(X), p(ip), p(ii), 2, p(W.Bsum), p(W.Amean), C.byref(par), NITER]
        assert lib.poismf_hip_session_factors_new(*lead, p(fac)) == 2, (indptr, indices)
        assert lib.poismf_hip_session_topn_new(*lead, 5, 1, None, None, p(out), p(sc), p(fac)) == 2, (indptr, indices)
        assert lib.poismf_hip_session_rank_new(*lead, p(held_p), p(held_i), 1, None, None, p(rk), p(na), p(fac)) == 2, (indptr, indices)
    # valid rows from here on: {4, 9} and {7}
    ip, ii = _u([0, 2, 3]), _u([4, 9, 7])
    lead = [W.sess.h, p(X), p(ip), p(ii), 2, p(W.Bsum), p(W.Amean), C.byref(par), NITER]
    assert lib.poismf_hip_session_factors_new(W.sess.h, None, p(ip), p(ii), 2, p(W.Bsum), p(W.Amean), C.byref(par), NITER, p(fac)) == 2   # no values
    for n in (0, 129, DIMB + 1):
        assert lib.poismf_hip_session_topn_new(*lead, n, 1, None, None, p(out), p(sc), p(fac)) == 2, n
    assert np.all(out == 12345) and np.all(sc == -7.0) and np.all(fac == -7.0) and np.all(rk == 12345) and np.all(na == 12345)
    # required outputs, and the lists' own checks
    assert lib.poismf_hip_session_factors_new(*lead, None) == 2
    assert lib.poismf_hip_session_topn_new(*lead, 5, 1, None, None, None, None, p(fac)) == 2
    assert lib.poismf_hip_session_rank_new(*lead, p(ip), p(ii), 1, None, None, None, None, p(fac)) == 2
    ep, ei = _u([0, 2, 4]), _u([1, 2, 9, 7])   # a descending exclusion row; the held-out rows {4, 9}, {7} are fine
    out, rk, na = np.full((2, 5), 12345, np.uint64), np.full(3, 12345, np.uint32), np.full(2, 12345, np.uint32)
    assert lib.poismf_hip_session_topn_new(*lead, 5, 1, p(ep), p(ei), p(out), None, p(fac)) == 2
    assert lib.poismf_hip_session_rank_new(*lead, p(ip), p(ii), 1, p(ep), p(ei), p(rk), p(na), p(fac)) == 2
    tp, ti = _u([0, 2, 3]), _u([9, 4, 7])     # a descending held-out row
    assert lib.poismf_hip_session_rank_new(*lead, p(tp), p(ti), 1, None, None, p(rk), p(na), p(fac)) == 2
    assert np.all(out == 12345) and np.all(rk == 12345) and np.all(na == 12345) and np.all(fac == -7.0)
    # too few left only once the row's own items are counted: 5990 listed + 2 own leave 8 of 6000
    ep, ei = _u([0, 5990, 5990]), _u(np.arange(10, 6000))
    out = np.full((2, 9), 12345, np.uint64)
    assert lib.poismf_hip_session_topn_new(*lead, 9, 1, p(ep), p(ei), p(out), None, p(fac)) == 2
    assert np.all(out == 12345) and np.all(fac == -7.0)
    assert lib.poismf_hip_session_topn_new(*lead, 8, 1, p(ep), p(ei), p(out), None, p(fac)) == 0
    assert sorted(out[0, :8].tolist()) == [0, 1, 2, 3, 5, 6, 7, 8]
