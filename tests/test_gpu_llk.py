"""The Poisson log-likelihood on the GPU (include/poismf_hip.h section 1e: eval_llk, poismf_hip_session_llk) against a float64
restatement: yhat by chunked einsum on the factors cast to float64, sums by math.fsum, math.lgamma.  The reference declares
eval_llk and defines it nowhere, so this restatement is the checker.  Needs an MI355X."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-12
FLAVOURS = [pytest.param(False, id="f64"), pytest.param(True, id="f32")]


def restated(A, B, X, full_llk=False, include_missing=False, chunk=1 << 18):
    """float64 restatement of section 1e; X: SciPy matrix or synth.Triplets with values already in the model's precision"""
    coo = sp.coo_matrix((np.asarray(X.data), (np.asarray(X.row), np.asarray(X.col))), shape=(A.shape[0], B.shape[0]))
    coo.sum_duplicates()   # (in the values' own precision, as the device conversion does)
    r, c, x = coo.row, coo.col, coo.data.astype(np.float64)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    yhat = np.empty(len(x))
    for lo in range(0, len(x), chunk):
        hi = min(len(x), lo + chunk)
        yhat[lo:hi] = np.einsum("ij,ij->i", A64[r[lo:hi]], B64[c[lo:hi]])
    with np.errstate(divide="ignore", invalid="ignore"):
        xlog = np.where(x != 0, x * np.log(yhat), 0.0)
    terms = [math.fsum(xlog)]
    if full_llk:
        terms.append(-math.fsum(math.lgamma(v + 1.0) for v in x))
    if include_missing:
        terms.append(-math.fsum(math.fsum(A64[:, j]) * math.fsum(B64[:, j]) for j in range(A.shape[1])))
    else:
        terms.append(-math.fsum(yhat))
    return math.fsum(terms)


def close(got, want):
    if math.isinf(want) or math.isnan(want):
        return got == want or (math.isnan(got) and math.isnan(want))
    return abs(got - want) <= RTOL * abs(want)


def model_with(A, B):
    """a PoisMF holding the given factors as if fitted"""
    m = api.PoisMF(k=A.shape[1], use_float=A.dtype == np.float32)
    m.A, m.B = A, B
    m.nusers, m.nitems = A.shape[0], B.shape[0]
    m.is_fitted = True
    return m


def random_factors(dimA, dimB, k, use_float, seed):
    rng = np.random.default_rng(seed)
    dt = np.float32 if use_float else np.float64
    return rng.uniform(0.05, 1.0, (dimA, k)).astype(dt), rng.uniform(0.05, 1.0, (dimB, k)).astype(dt)


def check_all(m, X):
    for full in (False, True):
        for miss in (False, True):
            got = m.eval_llk(X, full_llk=full, include_missing=miss)
            want = restated(m.A, m.B, X, full, miss)
            assert math.isfinite(want)
            assert close(got, want), (full, miss, got, want, abs(got - want) / abs(want))


def _split(coo, seed=3):
    rng = np.random.default_rng(seed)
    test = rng.random(coo.nnz) < 0.2
    mk = lambda msk: sp.coo_matrix((coo.data[msk], (coo.row[msk], coo.col[msk])), shape=coo.shape)
    return mk(~test), mk(test)


@pytest.mark.parametrize("use_float", FLAVOURS)
@pytest.mark.parametrize("method", ["pg", "cg", "tncg"])
def test_c1_fitted_train_and_heldout(use_float, method):
    train, test = _split(synth.readme_coo())
    kw = dict(l2_reg=1e3, initial_step=1e-9) if method == "pg" else {}   # (PG's defaults drive every factor to exact zero here)
    m = api.PoisMF(k=5, method=method, use_float=use_float, niter=5, **kw).fit(train)
    dt = np.float32 if use_float else np.float64
    for X in (train, test):
        X = sp.coo_matrix((X.data.astype(dt), (X.row, X.col)), shape=X.shape)
        check_all(m, X)


@pytest.mark.parametrize("use_float", FLAVOURS)
def test_c2_sized(use_float):
    t = synth.uniform_triplets(10 ** 5, 10 ** 5, 10 ** 7, seed=5)
    dt = np.float32 if use_float else np.float64
    t = synth.Triplets(t.row, t.col, t.data.astype(dt), t.shape)
    A, B = random_factors(10 ** 5, 10 ** 5, 50, use_float, 6)
    m = model_with(A, B)
    for full, miss in ((False, False), (True, True)):
        got = m.eval_llk(t, full_llk=full, include_missing=miss)
        want = restated(A, B, t, full, miss)
        assert close(got, want), (full, miss, got, want)


def medium_triplets(dimA, dimB, nnz, use_float, seed, long_rows=((7, 20000), (8, 9000))):
    """uniform triplets plus rows far longer than one range of the kernel (4096 nonzeros), an empty user and an empty item"""
    rng = np.random.default_rng(seed)
    row = [rng.integers(0, dimA, nnz)]
    col = [rng.integers(0, dimB, nnz)]
    for r, n in long_rows:
        row.append(np.full(n, r))
        col.append(rng.permutation(dimB)[:n])
    row, col = np.concatenate(row), np.concatenate(col)
    keep = (row != dimA - 1) & (col != 3)
    row, col = row[keep], col[keep]
    val = 1.0 + np.floor(rng.gamma(1.0, 1.0, len(row)))
    return synth.Triplets(row.astype(np.int64), col.astype(np.int64), val.astype(np.float32 if use_float else np.float64), (dimA, dimB))


@pytest.mark.parametrize("use_float", FLAVOURS)
@pytest.mark.parametrize("k", [1, 5, 100, 200])
def test_medium_k(use_float, k):
    t = medium_triplets(3000, 25000, 300000, use_float, seed=k)
    A, B = random_factors(3000, 25000, k, use_float, seed=k + 1)
    check_all(model_with(A, B), t)


@pytest.mark.parametrize("use_float", FLAVOURS)
def test_repeatable_and_session_bits(use_float):
    t = medium_triplets(3000, 25000, 300000, use_float, seed=11)
    A, B = random_factors(3000, 25000, 50, use_float, seed=12)
    m = model_with(A, B)
    sess = api.Session.from_coo(t, 50, use_float)
    try:
        sess.set_factors(A, B)
        for full in (False, True):
            for miss in (False, True):
                a = m.eval_llk(t, full, miss)
                assert m.eval_llk(t, full, miss) == a
                s = sess.llk(full, miss)
                assert sess.llk(full, miss) == s
                assert np.float64(s).tobytes() == np.float64(a).tobytes(), (full, miss, s, a)
    finally:
        sess.close()


@pytest.mark.parametrize("use_float", FLAVOURS)
def test_session_follows_its_factors(use_float):
    t = medium_triplets(2000, 5000, 100000, use_float, seed=21, long_rows=((1, 4500),))
    A, B = random_factors(2000, 5000, 20, use_float, seed=22)
    sess = api.Session.from_coo(t, 20, use_float)
    try:
        sess.set_factors(A, B)
        before = sess.llk()
        # the session's own row kernels write A (the padded gather copies follow them)
        p = sess.make_params("pg", 1e3, step_size=1e-9)
        sess.half_sweep(1, p, sess.real(1e-9), sess.cnst_div(1e3, 1e-9))
        A1, B1 = sess.get_factors()
        assert not np.array_equal(A1, A)
        assert sess.llk() == model_with(A1, B1).eval_llk(t)
        # set_factors from the host
        A2, B2 = random_factors(2000, 5000, 20, use_float, seed=23)
        sess.set_factors(A2, B2)
        got = sess.llk(True, True)
        assert got != before and close(got, restated(A2, B2, t, True, True))
        sess.factors_dirty(1)
        sess.factors_dirty(0)
        assert sess.llk(True, True) == got
    finally:
        sess.close()


@pytest.mark.parametrize("use_float", FLAVOURS)
def test_edge_cases(use_float):
    dt = np.float32 if use_float else np.float64
    A, B = random_factors(5, 7, 3, use_float, seed=31)
    m = model_with(A, B)
    T = lambda r, c, v: synth.Triplets(np.array(r, np.int64), np.array(c, np.int64), np.array(v, dt), (5, 7))
    # no cells: 0, or -M
    empty = T([], [], [])
    assert m.eval_llk(empty) == 0.0 and m.eval_llk(empty, full_llk=True) == 0.0
    assert close(m.eval_llk(empty, include_missing=True), restated(A, B, empty, False, True))
    # an explicit x = 0 cell costs its yhat only
    yhat = float(np.dot(A[1].astype(np.float64), B[2].astype(np.float64)))
    z = T([1], [2], [0.0])
    assert close(m.eval_llk(z), -yhat) and close(m.eval_llk(z, full_llk=True), -yhat)
    # duplicates are summed first: the same bits as the summed cell
    assert m.eval_llk(T([1, 0, 1], [2, 4, 2], [2.0, 1.0, 3.0]), True) == m.eval_llk(T([0, 1], [4, 2], [1.0, 5.0]), True)
    # users and items without cells, all four flavours of the sum
    check_all(m, T([0, 2, 2, 3], [1, 1, 5, 0], [1.0, 4.0, 2.0, 7.0]))
    # an all-zero user with x > 0: -inf
    A0 = A.copy()
    A0[2] = 0
    assert m.eval_llk(T([2], [3], [1.0])) != -np.inf   # (the model's own factors are positive)
    assert model_with(A0, B).eval_llk(T([0, 2], [3, 3], [1.0, 1.0])) == -np.inf
    # a NaN factor: NaN
    An = A.copy()
    An[4, 1] = np.nan
    assert math.isnan(model_with(An, B).eval_llk(T([4, 0], [0, 1], [2.0, 1.0])))
    assert math.isnan(model_with(An, B).eval_llk(T([0], [1], [1.0]), include_missing=True))
