"""explain (include/poismf_hip.h section 1v) on the GPU against the definition in plain numpy: an exact world of small integers
compared bit for bit -- which is also the test of the order rule (many ties) and of the zero rule (rows of B orthogonal to the
user) --, random positive factors against float64 within the chains' rounding bound, and the session against the host entry."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api

pytestmark = pytest.mark.gpu

DIMB = 1200
DT = {True: np.float32, False: np.float64}


def _slice(m, is_float):
    return int(api.load_library(is_float).poismf_hip_explain_slice(1, m))


def _seen(rng, lengths, dt):
    """one strictly ascending row of each length, counts 1..8: (indptr, indices, values)"""
    rows = [np.sort(rng.choice(DIMB, n, replace=False)) for n in lengths]
    indices = np.concatenate(rows).astype(np.uint64)
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64), indices, rng.integers(1, 9, len(indices)).astype(dt)


def _pages(rng, n_users, n_q):
    """distinct query items per user; the second user's page is padded with TOPN_NONE from its middle on"""
    q = np.stack([rng.choice(DIMB, n_q, replace=False) for _ in range(n_users)]).astype(np.uint64)
    q[1, n_q // 2:] = api.TOPN_NONE
    return q


def _definition(A, B, users, q, seen, g, m, dt):
    """section 1v in `dt`, one operation at a time: (items, contributions, every seen item's contribution per cell)"""
    indptr, indices, x = (np.asarray(v) for v in seen)
    ix = np.full(q.shape + (m,), api.TOPN_NONE, np.uint64)
    val = np.full(q.shape + (m,), -np.inf, dt)
    full = {}
    for i, u in enumerate(users):
        rows = indices[int(indptr[i]):int(indptr[i + 1])].astype(np.int64)
        a, Bs, xs = A[u].astype(dt), B[rows].astype(dt), x[int(indptr[i]):int(indptr[i + 1])].astype(dt)
        d = Bs @ a
        for t, j in enumerate(q[i]):
            if j == api.TOPN_NONE:
                continue
            qc = ((a * g) * B[int(j)].astype(dt)).astype(dt)
            with np.errstate(divide="ignore", invalid="ignore"):
                v = ((xs * (Bs @ qc)).astype(dt) / d).astype(dt)
            v[(d == 0) | ~np.isfinite(v)] = 0
            order = np.lexsort((rows, -v))[:m]
            ix[i, t, :len(order)], val[i, t, :len(order)], full[i, t] = rows[order], v[order], dict(zip(rows, v))
    return ix, val, full


@pytest.mark.parametrize("m", [1, 5, 64])
@pytest.mark.parametrize("n_q", [1, 15, 16, 17])
@pytest.mark.parametrize("k", [1, 3, 4, 50, 67])
@pytest.mark.parametrize("is_float", [True, False])
def test_exact_world_bit_for_bit(is_float, k, n_q, m):
    """integers 0..7 with zeros enough that d_i = 0 occurs, counts 1..8, g None or powers of two: every chain is exact
    (x * num <= 8 * 67 * 7^3 * 4 < 2^24), so items and contribution bits are compared with no tolerance"""
    dt, rng = DT[is_float], np.random.default_rng(1000 * k + 10 * n_q + m)
    lengths = [0, 1, 15, 16, 17, 63, 64, 65, 130, _slice(m, is_float) + 1]
    A = (rng.integers(0, 8, (len(lengths), k)) * (rng.random((len(lengths), k)) < 0.6)).astype(dt)
    B = (rng.integers(0, 8, (DIMB, k)) * (rng.random((DIMB, k)) < (0.5 if k > 4 else 0.7))).astype(dt)
    B[::5, : (k + 1) // 2] = 0   # with the line below, every fifth item is orthogonal to the first users
    A[:5, (k + 1) // 2:] = 0
    users = np.arange(len(lengths), dtype=np.uint64)
    seen, q = _seen(rng, lengths, dt), _pages(rng, len(users), n_q)
    g = None if k in (1, 50) else (2.0 ** rng.integers(-1, 3, k)).astype(dt)
    want_ix, want_val, _ = _definition(A, B, users, q, seen, dt(1) if g is None else g, m, dt)
    ix, val = api.explain(A, B, users, q, seen, m=m, comp_scale=g)
    assert np.array_equal(ix, want_ix)
    assert np.array_equal(val.view(np.uint8), want_val.view(np.uint8))


@pytest.mark.parametrize("is_float", [True, False])
def test_random_factors_against_float64(is_float):
    """k = 50, rows of 100 and of one slice + 1: the sorted contributions position by position, and every returned item's own
    float64 contribution, within (2 k + 8) u -- two k-term chains of non-negative terms plus the five single roundings"""
    dt, k, m, rng = DT[is_float], 50, 5, np.random.default_rng(7)
    lengths = [100, _slice(m, is_float) + 1, 100]
    A, B = rng.gamma(1.0, 0.5, (len(lengths), k)).astype(dt), rng.gamma(1.0, 0.5, (DIMB, k)).astype(dt)
    users = np.arange(len(lengths), dtype=np.uint64)
    seen, q, g = _seen(rng, lengths, dt), _pages(rng, len(users), 10), (1.0 / (B.sum(0, dtype=np.float64) + 0.1)).astype(dt)
    ix, val = api.explain(A, B, users, q, seen, m=m, comp_scale=g)
    want_ix, want_val, full = _definition(A, B, users, q, seen, g.astype(np.float64), m, np.float64)
    tol = (2 * k + 8) * 2.0 ** (-24 if is_float else -53)
    assert np.array_equal(ix == api.TOPN_NONE, want_ix == api.TOPN_NONE)
    real = ix != api.TOPN_NONE
    assert np.all(np.abs(val[real] - want_val[real]) <= tol * want_val[real])
    for i, t, r in zip(*np.nonzero(real)):
        own = full[i, t][int(ix[i, t, r])]
        assert abs(float(val[i, t, r]) - own) <= tol * own


@pytest.mark.parametrize("is_float", [True, False])
def test_session_against_host_entry(is_float):
    """the resident rows and factors give the host entry's bits, and a user's cells do not depend on the batch around it"""
    dt, k, rng = DT[is_float], 50, np.random.default_rng(11)
    lengths = [100, 3, _slice(5, is_float) + 1, 64, 1]
    indptr, indices, x = _seen(rng, lengths, dt)
    coo = sp.csr_matrix((x, indices.astype(np.int64), indptr.astype(np.int64)), shape=(len(lengths), DIMB)).tocoo()
    A, B = rng.gamma(1.0, 0.5, (len(lengths), k)).astype(dt), rng.gamma(1.0, 0.5, (DIMB, k)).astype(dt)
    s = api.Session.from_coo(coo, k, is_float)
    s.set_factors(A, B)
    users, q = np.arange(len(lengths), dtype=np.uint64), _pages(rng, len(lengths), 17)
    val_s, ind_s, ptr_s = s.matrix(1)
    got = s.explain(users, q, m=5)
    host = api.explain(A, B, users, q, (ptr_s, ind_s, val_s), m=5)
    alone = [s.explain(users[i:i + 1], q[i:i + 1], m=5) for i in range(len(users))]
    s.close()
    for a, b in zip(got, host):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for i, one in enumerate(alone):
        assert np.array_equal(one[0][0], got[0][i]) and np.array_equal(one[1][0].view(np.uint8), got[1][i].view(np.uint8))
