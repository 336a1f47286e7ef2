"""Method "mm" (include/poismf_hip.h section 0; solvers.hpp, mm_row) on the GPU against the update written out in numpy float64 (mm_ref).

One small matrix per k.  Its A rows have 0, 1, 15, 16, 17, 64, 65 nonzeros (one-wave register kernels; the quad engine at k = 50 fp32) and four lengths read off
api.debug_plan(..., "mm", engines=True): 300 (half_sweep_regw_kernel), 600 (half_sweep_lane_kernel at k = 50 fp32), 1300 (one-wave half_sweep_kernel) and 8300 (its
eight-wave streamed instance); k = 100 and k = 50 fp64 run the LDS kernels, resident and streamed, and the two-slot register kernels on them."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness

pytestmark = pytest.mark.gpu
FLOOR, DIMB, LENGTHS = 1e-10, 8400, [0, 1, 15, 16, 17, 64, 65, 300, 600, 1300, 8300]
# per-row error max_c |a - ref| / max_c |ref|: PG's bounds against the oracle (tests/test_gpu_parity.py) hold as they stand.  Measured here, the largest over every case
# of test_against_float64: fp64 6.7e-14, fp32 3.2e-6 (k = 100, w = 3, l2 = 0, ten updates; the 8300- and the 1300-nonzero row); one update: 1.1e-14 / 7.4e-7
BOUND = {False: 1e-12, True: 1e-5}
both = pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])


def problem(k, use_float):
    """[(column indices, counts)] per A row, A0, B -- values in the model's precision"""
    rng, dt = np.random.default_rng(7 + k), np.float32 if use_float else np.float64
    rows = [(np.sort(rng.choice(DIMB, n, replace=False)), (1 + np.floor(rng.standard_gamma(1.0, n))).astype(dt)) for n in LENGTHS]
    return rows, (0.3 + rng.uniform(0, 0.3, (len(LENGTHS), k))).astype(dt), (0.05 + rng.uniform(0, 0.5, (DIMB, k))).astype(dt)


def mm_ref(rows, A0, B, bsum, w, l2, maxupd):
    """the update in float64: (A, updates made per row, the row objective fun_single before, after)"""
    A, B, made, f0, f1 = np.array(A0, np.float64), np.asarray(B, np.float64), np.zeros(len(A0), np.int64), np.zeros(len(A0)), np.zeros(len(A0))
    row_f = lambda a, Bj, x, s: s @ a + l2 * a @ a - w * np.sum(x * np.log(Bj @ a))
    for r, (j, x) in enumerate(rows):
        if len(j) == 0:
            A[r] = 0
            continue
        s, a, x = np.asarray(bsum, np.float64) + (w - 1.) * B[j].sum(0), np.where(A[r] > FLOOR, A[r], FLOOR), x.astype(np.float64)
        with np.errstate(all="ignore"):
            f0[r] = row_f(a, B[j], x, s)
            for _ in range(maxupd):
                m = w * a * ((x / (B[j] @ a)) @ B[j])
                new = np.where(m == 0, 0., 2 * m / (s + np.sqrt(s * s + 8 * l2 * m)))
                if not np.isfinite(new).all():
                    break
                a, made[r] = new, made[r] + 1
            A[r], f1[r] = a, row_f(a, B[j], x, s)
    return A, made, f0, f1


def row_err(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-300)))


def csr_of(rows, dt):
    return (np.concatenate([x for _, x in rows]).astype(dt), np.concatenate([j for j, _ in rows]).astype(np.uint64),
            np.concatenate([[0], np.cumsum([len(j) for j, _ in rows])]).astype(np.uint64))


def half_sweep(rows, A0, B, w, l2, maxupd):
    """the A half of a session on these rows: (A, updates made per row)"""
    val, ind, ptr = csr_of(rows, A0.dtype)
    c, cc = harness.process_data(sp.csr_matrix((val, ind.astype(np.int64), ptr.astype(np.int64)), shape=(len(A0), DIMB)), A0.dtype == np.float32)
    s = api.Session(c, cc, len(A0), DIMB, A0.shape[1], A0.dtype == np.float32)
    try:
        s.set_factors(A0, B)
        s.profile(True)
        s.half_sweep(1, s.make_params("mm", l2, 0.0, w, maxupd=maxupd), 1e-7, 1.0)
        return s.get_factors()[0], s.decisions(1)[0]
    finally:
        s.close()


@pytest.mark.parametrize("maxupd", [1, 10])
@pytest.mark.parametrize("l2", [0., 1e3])
@pytest.mark.parametrize("w", [1., 3.])
@pytest.mark.parametrize("k", [3, 50, 100])
@both
def test_against_float64(use_float, k, w, l2, maxupd):
    rows, A0, B = problem(k, use_float)
    bsum = B.astype(np.float64).sum(0)
    got, made = half_sweep(rows, A0, B, w, l2, maxupd)
    e1 = row_err(got, mm_ref(rows, A0, B, bsum, w, l2, maxupd)[0])
    # factors_multiple: every row starts at Amean, niter * maxupd updates in one half-sweep
    amean, bs, (val, ind, ptr) = A0.mean(0).astype(A0.dtype), bsum.astype(A0.dtype), csr_of(rows, A0.dtype)
    got2 = api._predict_factors_multiple(B, bs, amean, ptr, ind, val, l2, w, 1e-7, 1, maxupd, "mm", True, True)
    e2 = row_err(got2, mm_ref(rows, np.tile(amean, (len(A0), 1)), B, bs, w, l2, maxupd)[0])
    print(f"mm {'f32' if use_float else 'f64'} k={k} w={w} l2={l2} maxupd={maxupd}: half_sweep {e1:.3g} factors_multiple {e2:.3g}")
    assert np.all(got[0] == 0) and np.all(got2[0] == 0) and got.min() >= 0 and got2.min() >= 0       # (row 0 is the empty one)
    assert np.array_equal(made[1:], np.full(len(A0) - 1, maxupd))
    assert e1 <= BOUND[use_float] and e2 <= BOUND[use_float]


@pytest.mark.parametrize("w,l2", [(1., 0.), (1., 1e3), (3., 1e3)])
@pytest.mark.parametrize("k", [3, 50, 100])
def test_one_update_descends_and_keeps_the_row_total(k, w, l2):
    rows, A0, B = problem(k, False)
    got, _ = half_sweep(rows, A0, B, w, l2, 1)
    _, _, before, _ = mm_ref(rows, A0, B, B.sum(0), w, l2, 0)
    _, _, after, _ = mm_ref(rows, got, B, B.sum(0), w, l2, 0)        # (no update: the objective at the returned factors)
    assert np.all(after <= before + 1e-12 * np.abs(before)), (after - before).max()
    if l2 == 0 and w == 1:   # the classical fixed point: a' = a r / s, so a'.s = sum_j x_j
        total, nnz = np.array([x.sum() for _, x in rows[1:]]), np.array(LENGTHS[1:])
        assert np.all(np.abs(got[1:] @ B.sum(0) - total) <= 1e-12 * nnz * total)


@both
def test_the_rules(use_float):
    """rows that start at zero fit from the floor; a row that meets an all-zero item keeps its point and reports no update; the empty row is zero"""
    rows, A0, B = problem(50, use_float)
    A0[[1, 3, 7, 9]] = 0
    B[rows[5][0][0]] = 0                                          # an item of the 64-nonzero row (and of whichever long rows drew it too)
    ref, made_ref, _, _ = mm_ref(rows, A0, B, B.astype(np.float64).sum(0), 1., 1e3, 10)
    got, made = half_sweep(rows, A0, B, 1., 1e3, 10)
    assert made_ref[5] == 0 and set(made_ref[[1, 2, 3, 4]]) == {10} and np.array_equal(made, made_ref), (made, made_ref)
    assert np.array_equal(got[5], A0[5]) and np.isfinite(got).all() and np.all(got[0] == 0) and got[[1, 3]].max(1).min() > 0
    assert row_err(got, ref) <= BOUND[use_float]


def test_fit_with_the_class_defaults():
    # (counts around 2000: the default l2_reg, CG's 1e4, holds a row's factors near sqrt(row total / 2e4) -- smaller totals are shrunk away, under "cg" too)
    rng, nu, ni = np.random.default_rng(3), 300, 200
    rate = rng.gamma(2., 1., (nu, 4)) @ rng.gamma(2., 1., (4, ni))
    X = sp.coo_matrix(rng.poisson(2000. * rate / rate.mean()).astype(np.float64))
    model, start = api.PoisMF(method="mm").fit(X), api.PoisMF(method="mm")
    assert (model.l2_reg_, model.niter_, model.maxupd_) == (1e4, 30, 10) and np.isfinite(model.A).all() and np.isfinite(model.B).all()
    assert model.A.min() >= 0 and model.B.min() >= 0 and model.A.max() > 0 and model.B.max() > 0
    start.A, start.B = harness.initialize_matrices(nu, ni, 50, True, 1)
    start.nusers, start.nitems, start.is_fitted = nu, ni, True
    assert model.eval_llk(X) > start.eval_llk(X)
