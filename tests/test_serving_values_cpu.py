"""The reference of tests/test_gpu_serving_values.py (tests/serving_values.py) meets, on its own and without a device, the conditions
the GPU test relies on: in every regime, precision and k the score chain emulated in real_t is exact in three summation orders -- so
the integer product is the expectation of every entry point, bit for bit -- the subnormal regimes are subnormal, `huge` stays finite,
`overflow` gives both infinities and no NaN, and the fixed users are what their names say."""
import numpy as np
import pytest

from poismf_amd import api
from tests import serving_values as V


@pytest.fixture(scope="module", params=V.CASES, ids=V.case_id)
def w(request):
    return V.world(*request.param)


ROWS = np.r_[0:8, 8:V.DIMA:5]      # the users whose chains are emulated step by step: the fixed ones and every fifth of the rest


def _step(w, s, c):
    """one step of the chain in real_t: the product rounded, then the sum rounded.  The fused step rounds the exact a b + s once; where
    this one stays on the exact integers at every step (the callers compare all of them), both are exact."""
    p = np.multiply(w.A[ROWS, c][:, None], w.B[:, c][None, :])
    assert p.dtype == w.dt
    return np.add(s, p)


def _partial(w, cols):
    """the exact partial score over the columns `cols`: an integer times 2^(eA + eB), and +-inf where `overflow` has met column 0"""
    e = w.Ai[np.ix_(ROWS, cols)] @ w.Bi[:, cols].T
    p = np.ldexp(e.astype(np.float64), w.eA + w.eB).astype(w.dt)
    assert np.array_equal(np.ldexp(p.astype(np.float64), -(w.eA + w.eB)), e), "a partial sum is not representable in real_t"
    if w.regime == "overflow" and 0 in cols:
        rows = np.flatnonzero(w.sign0[ROWS])
        p[np.ix_(rows, V.J)] = np.where(w.sign0[ROWS][rows] > 0, np.inf, -np.inf).astype(w.dt)[:, None]
    return p


def _chain(w, cols):
    """the chain over `cols` in this order, every partial sum compared with the exact one"""
    s = np.zeros((len(ROWS), V.DIMB), w.dt)
    done = []
    with np.errstate(over="ignore"):
        for c in cols:
            s = _step(w, s, c)
            done.append(c)
            assert s.dtype == w.dt
            assert np.array_equal(V.bits(s + w.dt(0)), V.bits(_partial(w, done))), (w.regime, w.is_float, w.k, "column", c)
    return s


def test_the_chain_is_exact_in_three_orders(w):
    k = w.k
    up = _chain(w, list(range(k)))
    down = _chain(w, list(range(k - 1, -1, -1)))
    # topN's order: sixteen strided partial chains, summed by a butterfly
    part = [_chain(w, list(range(i, k, 16))) for i in range(16)]
    with np.errstate(over="ignore"):
        for off in (8, 4, 2, 1):
            part = [np.add(part[i], part[i ^ off]) for i in range(16)]
    for what, s in (("ascending", up), ("descending", down), ("strided", part[0])):
        ok = np.array_equal(V.bits(s + w.dt(0)), V.bits(w.S[ROWS]))
        print(f"{V.case_id((w.regime, w.is_float, w.k))} {what}: equal bits {ok}")
        assert ok, what
    assert all(np.array_equal(V.bits(p), V.bits(part[0])) for p in part)


def test_the_regime_is_what_it_says(w):
    S, fi = w.S, np.finfo(w.dt)
    assert not np.isnan(S).any()
    if w.regime in V.SUBNORMAL:
        a = np.abs(S)
        nonzero = float((a > 0).mean())
        print(f"{V.case_id((w.regime, w.is_float, w.k))}: largest |s| / tiny {float(a.max()) / float(fi.tiny):.3g}, nonzero {nonzero:.4f}")
        assert (a < fi.tiny).all() and nonzero > 0.9
        sub = lambda M: (np.abs(M[M != 0]) < fi.tiny).all() and (M != 0).any()
        nrm = lambda M: (np.abs(M[M != 0]) >= fi.tiny).all()
        assert {"sub_out": nrm(w.A) and nrm(w.B), "sub_a": sub(w.A) and nrm(w.B), "sub_b": nrm(w.A) and sub(w.B)}[w.regime]
    elif w.regime == "overflow":
        assert np.isposinf(S).any(axis=1).any() and np.isneginf(S).any(axis=1).any()
        assert np.isfinite(w.A).all() and np.isfinite(w.B).all()
        finite = np.isfinite(S)
        assert (~finite).sum() == np.count_nonzero(w.sign0) * len(V.J)
        assert np.array_equal(S[finite], w.Ei[finite].astype(w.dt))
    else:
        assert np.isfinite(S).all()
        if w.regime == "huge":
            assert float(np.abs(S).max()) > 2.0 ** 100 or w.k == 1
    if w.regime == "sparse":
        zeros = (S == 0).sum(axis=1)
        print(f"{V.case_id((w.regime, w.is_float, w.k))}: scores of exactly 0 per user: fewest {zeros.min()}, median {int(np.median(zeros))}")
        assert zeros.min() > 50 and np.median(zeros) > (500 if w.k > 1 else 2000)
        assert (w.Ai[4:] >= 0).all() and (w.Bi >= 0).all() and (w.Bi == 0).mean(axis=0).min() > 0.8


def test_the_fixed_users(w):
    S = w.S
    assert (S[0] == 0).all() and not np.signbit(S[0]).any()
    if w.regime in ("sparse", "overflow"):      # (column 0 of B is not positive everywhere there)
        assert (S[1] <= 0).all() and (S[1] < 0).any() and (S[2] >= 0).all() and (S[2] > 0).any()
    else:
        assert (S[1] < 0).all() and (S[2] > 0).all()
        assert len(np.unique(S[1])) == 3 and np.unique(S[1], return_counts=True)[1].min() > 900
    adm = np.setdiff1d(np.arange(V.DIMB), w.extra[3])
    assert len(adm) == V.KEEP3 == api.TOPN_BATCH_MAX_N_TOP and np.isin(w.seen[3], w.extra[3]).all()
    assert adm.max() >= 3072, "none of user 3's items is in the last, partial tile"
    if w.regime == "overflow":
        assert np.isneginf(S[1, V.J]).all() and np.isposinf(S[2, V.J]).all()
        assert 5 <= np.isneginf(S[3, adm]).sum() < len(adm)


def test_the_lists_reach_the_edges(w):
    assert V.DIMA > 2 * 64 and V.DIMA % 64 and V.DIMB % 64 == 5
    assert sorted({len(l) for l in w.incl}) == sorted(V.INCLUDE_SIZES)
    assert all(len(l) == 0 or (np.diff(l) > 0).all() for rows in (w.seen, w.extra, w.incl, w.test, w.shared) for l in rows)
    assert sum(int(l.max() >= 3072) for l in w.incl if len(l)) > 50
    short = [u for u in range(V.DIMA) if 0 < len(w.incl[u]) <= 5]
    assert short and all(np.isin(w.incl[u], V.J).any() for u in short)
    assert np.array_equal(w.shared[0], np.arange(V.DIMB)) and all(np.isin(l, V.J).any() and l.max() >= 3072 for l in w.shared)
    for u in range(V.DIMA):
        assert np.isin(w.test[u], V.J).any()
        if len(w.extra[u]) >= 3:
            assert np.isin(w.test[u], w.extra[u]).any()


def test_the_expectation_functions_on_a_hand_written_row():
    w = V.world("signed", True, 1)
    users = [1, 2]
    m = w.mask(users, include=[[5, 9, 2, 3076], [4, 8]], exclude=[[9], []], unite=[[7], [8]])
    assert m.sum(axis=1).tolist() == [4, 2] and m[0, [2, 5, 7, 3076]].all() and m[1, [4, 8]].all()
    ix, sc = w.topn(users, m, 5)
    for i, u in enumerate(users):
        c = np.flatnonzero(m[i])
        best = sorted(c, key=lambda j: (-float(w.S[u, j]), j))
        assert ix[i, :len(c)].tolist() == best and (ix[i, len(c):] == api.TOPN_NONE).all()
        assert sc[i, :len(c)].tolist() == [float(w.S[u, j]) for j in best] and np.isneginf(sc[i, len(c):]).all()
    r, n_adm = w.ranks(users, m, [[2, 9, 3076], [8]])
    assert n_adm.tolist() == [4, 2] and r[1] == api.RANK_EXCLUDED
    assert [int(r[0]), int(r[2])] == [list(ix[0]).index(2), list(ix[0]).index(3076)] and int(r[3]) == list(ix[1]).index(8)
