"""The values the COO conversion stores for duplicate cells with non-integer triplets (include/poismf_hip.h section 1c), through every
caller of the conversion: api.coo_to_csr_csc, Session.from_coo with and without shards, Session.add and eval_llk.  The expectation is
tests/coo_values.py -- a cell's triplets summed in input order, every addition rounded in real_t -- never SciPy.  All equalities are on
bits.  Needs an MI355X."""
import types

import numpy as np
import pytest

from poismf_amd import api
from tests import coo_values as V
from tests.coo_values import Triplets, bits, reference_cs
from tests.test_gpu_llk import model_with, random_factors

pytestmark = pytest.mark.gpu
K = 8


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def dtype_of(prec):
    return np.float32 if prec else np.float64


def differing(got, want):
    """None when got = (values, indices, indptr) is the expected orientation; otherwise what differs, with the number of cells"""
    val, ind, ptr = got
    if not np.array_equal(np.asarray(ptr).astype(np.int64), want[2]):
        return "row pointers differ"
    if not np.array_equal(np.asarray(ind).astype(np.int64), want[1]):
        return "indices differ"
    if val.dtype != want[0].dtype:
        return f"values are {val.dtype}"
    bad = int((bits(val) != bits(want[0])).sum())
    return f"{bad} of {len(val)} cells differ in bits" if bad else None


def same(got, want, what):
    d = differing(got, want)
    assert d is None, f"{what}: {d}"


def both(t, dt):
    """(CSR, CSC) of the triplets by the rule"""
    return reference_cs(t.row, t.col, t.data, t.shape, dt, 0), reference_cs(t.row, t.col, t.data, t.shape, dt, 1)


@pytest.fixture(scope="module")
def W(prec):
    """the world, its reference in both orientations, and ONE conversion of it by api.coo_to_csr_csc"""
    dt = dtype_of(prec)
    w = V.world(dt, 11)
    csr, csc = both(w, dt)
    got = api.coo_to_csr_csc(w, prec)
    return types.SimpleNamespace(dt=dt, t=w, csr=csr, csc=csc, got=got)


# ---- T1, T2: the host entry point on the world ------------------------------------------------------------------------------------------
def test_t1_world_is_the_reference_and_inside_the_bound(prec, W):
    for name, major, got, want in (("CSR", 0, W.got[0], W.csr), ("CSC", 1, W.got[1], W.csc)):
        assert np.array_equal(got[2].astype(np.int64), want[2]) and np.array_equal(got[1].astype(np.int64), want[1]), name
        ratio = V.exact_and_bound(W.t.row, W.t.col, W.t.data, W.t.shape, W.dt, major, got=got[0])[2]
        print(f"{name}: worst |value - exact sum| / bound {ratio.max():.3f}; {int((bits(got[0]) != bits(want[0])).sum())} cells off the rule")
        assert ratio.max() <= 1.0, name          # (d - 1) u sum|t|: holds for any order of the additions
    same(W.got[0], W.csr, "CSR")
    same(W.got[1], W.csc, "CSC")


def test_t2_csr_and_csc_hold_the_same_bits(prec, W):
    (rv, ri, rp), (cv, ci, cp) = W.got
    col = np.repeat(np.arange(len(cp) - 1), np.diff(cp.astype(np.int64)))
    order = np.argsort(ci.astype(np.int64), kind="stable")           # the CSC's entries, by row, columns ascending within a row
    assert np.array_equal(ci[order], np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))) and np.array_equal(col[order], ri.astype(np.int64))
    bad = int((bits(cv[order]) != bits(rv)).sum())
    assert bad == 0, f"{bad} of {len(rv)} cells differ between the CSR and the CSC"


# ---- T3, T4: sessions, whole and sharded ------------------------------------------------------------------------------------------------
def test_t3_session_from_coo_holds_the_reference(prec, W):
    s = api.Session.from_coo(W.t, K, prec)
    try:
        assert s.nnz(1) == s.nnz(0) == len(W.csr[0])
        same(s.matrix(1), W.csr, "CSR")
        same(s.matrix(0), W.csc, "CSC")
    finally:
        s.close()


CUTS = [(0, 1), (1, 128), (1, 129), (1, 130), (172, 300), (290, 300)]   # local dimensions 1, 127, 128, 129 (end_bit steps at 2^7); no triplet


@pytest.mark.parametrize("cut", CUTS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_t4_shard_holds_the_unsharded_rows(prec, W, cut):
    """A shard of the CSR holds the bits of the same rows of the whole matrix, and so does a shard of the CSC.  The cuts reach 300, so
    the CSC shards are cut from the transposed world (200 x 300): the same triplets in the same order, its columns the world's rows."""
    lo, hi = cut
    t = W.t
    a, b = W.csr[2][lo], W.csr[2][hi]
    rows_of_whole = (W.csr[0][a:b], W.csr[1][a:b], W.csr[2][lo:hi + 1] - a)
    want = reference_cs(t.row, t.col, t.data, t.shape, W.dt, 0, lo, hi)
    same(want, rows_of_whole, "the reference's own cut")
    s = api.Session.from_coo(t, K, prec, shardA=cut)
    try:
        assert s.nnz(1) == len(want[0]) and s.nnz(0) == len(W.csc[0])
        same(s.matrix(1), want, f"CSR shard {cut}")
        same(s.matrix(0), W.csc, "the CSC beside a CSR shard")
    finally:
        s.close()
    tt = Triplets(t.col, t.row, t.data, t.shape[::-1])
    want = reference_cs(tt.row, tt.col, tt.data, tt.shape, W.dt, 1, lo, hi)
    same(want, rows_of_whole, "the transposed reference's cut")
    s = api.Session.from_coo(tt, K, prec, shardB=cut)
    try:
        assert s.nnz(0) == len(want[0]) and s.nnz(1) == len(W.csc[0])
        same(s.matrix(0), want, f"CSC shard {cut}")
        same(s.matrix(1), W.csc, "the CSR beside a CSC shard")
    finally:
        s.close()


# ---- T5: a cell's bits do not depend on the other triplets of the call ------------------------------------------------------------------
def test_t5_probe_cells_keep_their_bits_behind_any_number_of_fillers(prec):
    dt = dtype_of(prec)
    rng = np.random.default_rng(17)
    dimA, dimB, n_probe = 40, 6000, 50
    cells = rng.choice((dimA - 10) * dimB, size=n_probe, replace=False)
    count = rng.integers(3, 41, n_probe)
    count[:2] = (3, 40)
    prow, pcol = np.repeat(10 + cells // dimB, count), np.repeat(cells % dimB, count)
    order = rng.permutation(len(prow))
    prow, pcol = prow[order], pcol[order]
    pval = rng.uniform(0.1, 9.0, len(prow)).astype(dt)
    fcol = rng.permutation(dimB)[:5000]                                    # fillers: single-triplet cells of row 0
    fval = rng.uniform(0.1, 9.0, 5000).astype(dt)
    want_csr, want_csc = both(Triplets(prow, pcol, pval, (dimA, dimB)), dt)
    first, off_rule = None, []
    for f in list(range(71)) + [5000]:
        t = Triplets(np.concatenate([np.zeros(f, np.int64), prow]), np.concatenate([fcol[:f], pcol]), np.concatenate([fval[:f], pval]), (dimA, dimB))
        csr, csc = api.coo_to_csr_csc(t, prec)
        assert len(csr[0]) == n_probe + f and np.array_equal(csr[1][f:].astype(np.int64), want_csr[1])
        probes = csc[1] >= 10
        assert probes.sum() == n_probe and np.array_equal(csc[1][probes].astype(np.int64), want_csc[1])
        got = (bits(csr[0][f:]).copy(), bits(csc[0][probes]).copy())
        first = first or got
        for name, g, g0, w_ in (("CSR", got[0], first[0], want_csr[0]), ("CSC", got[1], first[1], want_csc[0])):
            if not np.array_equal(g, g0):
                off_rule.append(f"{name} f={f}: {int((g != g0).sum())} probe cells differ from f=0")
            if not np.array_equal(g, bits(w_)):
                off_rule.append(f"{name} f={f}: {int((g != bits(w_)).sum())} probe cells off the rule")
    assert not off_rule, f"{len(off_rule)} findings, the first: {off_rule[:6]}"


# ---- T6: a cell far longer than one block of any reduction -----------------------------------------------------------------------------
def test_t6_hot_cell_three_times(prec):
    """One cell with 200 000 triplets among 1000 others: three fresh conversions give the same bits, the reference's, inside the bound.
    How a run that spans several blocks is associated by a decoupled look-back depends on timing, which a test cannot force: this pins
    the property (the sequential rule leaves nothing to timing) more than it hunts any particular implementation."""
    dt = dtype_of(prec)
    rng = np.random.default_rng(23)
    dimA, dimB, hot, n_hot = 50, 60, (25, 30), 200000
    orow, ocol = rng.integers(0, dimA, 1000), rng.integers(0, dimB, 1000)
    keep = ~((orow == hot[0]) & (ocol == hot[1]))
    row = np.concatenate([orow[keep], np.full(n_hot, hot[0])])
    col = np.concatenate([ocol[keep], np.full(n_hot, hot[1])])
    order = rng.permutation(len(row))
    t = Triplets(row[order], col[order], rng.uniform(0.1, 9.0, len(row)).astype(dt), (dimA, dimB))
    want = both(t, dt)
    runs = [api.coo_to_csr_csc(t, prec) for _ in range(3)]
    for major, name in ((0, "CSR"), (1, "CSC")):
        ratio = V.exact_and_bound(t.row, t.col, t.data, t.shape, dt, major, got=runs[0][major][0])[2]
        print(f"{name}: worst |value - exact sum| / bound {ratio.max():.4f}")
        assert ratio.max() <= 1.0
        for i in (1, 2):
            assert np.array_equal(bits(runs[i][major][0]), bits(runs[0][major][0])), f"{name}: run {i} differs from run 0"
        same(runs[0][major], want[major], name)


# ---- T7: absorption ---------------------------------------------------------------------------------------------------------------------
def test_t7_absorption_follows_the_input_order(prec):
    dt = dtype_of(prec)
    big = float(V.big_of(dt))
    csr, csc = api.coo_to_csr_csc(V.absorption_triplets(dt), prec)
    assert csr[1].tolist() == [3, 1] and csr[2].tolist() == [0, 1, 1, 2, 2] and csr[0].tolist() == [big + 2.0, big]
    assert csc[1].tolist() == [2, 0] and csc[2].tolist() == [0, 0, 1, 1, 2, 2] and csc[0].tolist() == [big, big + 2.0]


# ---- T8: Session.add --------------------------------------------------------------------------------------------------------------------
def test_t8_add_sums_the_update_by_the_rule_then_adds_once(prec):
    dt = dtype_of(prec)
    rng = np.random.default_rng(29)
    dimA, dimB = 57, 83
    xcell = rng.choice(dimA * dimB, size=1500, replace=False)
    X = Triplets(xcell // dimB, xcell % dimB, rng.uniform(0.1, 9.0, 1500).astype(dt), (dimA, dimB))
    others = np.setdiff1d(np.arange(dimA * dimB), xcell)
    dcell = np.concatenate([rng.choice(xcell, size=400, replace=False), rng.choice(others, size=300, replace=False)])
    rep = rng.integers(1, 13, len(dcell))
    rep[:2] = (1, 12); rep[-2:] = (1, 12)
    dkey = np.repeat(dcell, rep)[rng.permutation(rep.sum())]
    D = Triplets(dkey // dimB, dkey % dimB, rng.uniform(0.1, 9.0, len(dkey)).astype(dt), (dimA, dimB))
    s = api.Session.from_coo(X, K, prec)
    try:
        assert s.add(D) == 300
        assert s.nnz(0) == s.nnz(1) == 1800
        for major, name in ((0, "CSR"), (1, "CSC")):
            xv, xi, xp = reference_cs(X.row, X.col, X.data, X.shape, dt, major)
            dv, di, dp = reference_cs(D.row, D.col, D.data, D.shape, dt, major)
            dim_minor = (dimB, dimA)[major]
            xk = np.repeat(np.arange(len(xp) - 1), np.diff(xp)) * dim_minor + xi
            dk = np.repeat(np.arange(len(dp) - 1), np.diff(dp)) * dim_minor + di
            keys = np.union1d(xk, dk)
            val = np.zeros(len(keys), dt)
            val[np.searchsorted(keys, xk)] = xv
            at = np.searchsorted(keys, dk)
            stored = np.isin(dk, xk)
            assert stored.sum() == 400
            val[at] = np.where(stored, val[at] + dv, dv)                  # x + s(D), one rounded addition; a new cell is s(D)
            ptr = np.zeros(len(xp), np.int64)
            np.cumsum(np.bincount(keys // dim_minor, minlength=len(xp) - 1), out=ptr[1:])
            same(s.matrix(1 - major), (val, keys % dim_minor, ptr), name + " after add")
    finally:
        s.close()


# ---- T9: the likelihood -----------------------------------------------------------------------------------------------------------------
def test_t9_llk_of_triplets_is_llk_of_the_summed_cells(prec, W):
    A, B = random_factors(W.t.shape[0], W.t.shape[1], K, prec, 31)
    m = model_with(A, B)
    summed = Triplets(np.repeat(np.arange(W.t.shape[0]), np.diff(W.csr[2])), W.csr[1], W.csr[0], W.t.shape)
    s1, s2 = api.Session.from_coo(W.t, K, prec), api.Session.from_coo(summed, K, prec)
    try:
        s1.set_factors(A, B); s2.set_factors(A, B)
        for full in (False, True):
            for miss in (False, True):
                a = m.eval_llk(W.t, full, miss)
                assert np.isfinite(a)
                assert m.eval_llk(W.t, full, miss) == a, (full, miss)
                assert m.eval_llk(summed, full, miss) == a, (full, miss)
                b = s1.llk(full, miss)
                assert s1.llk(full, miss) == b and s2.llk(full, miss) == b, (full, miss)
    finally:
        s1.close(); s2.close()


# ---- T10: shapes ------------------------------------------------------------------------------------------------------------------------
def _shape_cases():
    rng = np.random.default_rng(37)

    def rnd(n, dimA, dimB):
        return rng.integers(0, dimA, n), rng.integers(0, dimB, n), rng.uniform(0.1, 9.0, n), (dimA, dimB)

    cases = {"one-triplet": ([2], [1], [0.3], (4, 3)),
             "one-cell-1000": (np.full(1000, 3), np.full(1000, 2), rng.uniform(0.1, 9.0, 1000), (5, 4)),
             "1x500": rnd(3000, 1, 500), "500x1": rnd(3000, 500, 1)}
    for dimA in (1, 2, 3, 255, 256, 257):
        r, c, v, shape = rnd(40 + 4 * dimA, dimA, 3)
        r[:12] = 0; r[12:24] = dimA - 1                                    # the first and the last row, with duplicates
        p = rng.permutation(len(r))
        cases[f"dimA-{dimA}"] = (r[p], c[p], v, shape)
    r, c, v, shape = rnd(5000, 30, 20)
    up = np.lexsort((c, r))
    cases["sorted"] = (r[up], c[up], v, shape)
    cases["descending"] = (r[up][::-1], c[up][::-1], v, shape)
    return cases


SHAPE_CASES = _shape_cases()


@pytest.mark.parametrize("case", sorted(SHAPE_CASES))
def test_t10_shapes(prec, case):
    dt = dtype_of(prec)
    r, c, v, shape = SHAPE_CASES[case]
    t = Triplets(r, c, np.asarray(v).astype(dt), shape)
    want = both(t, dt)
    got = api.coo_to_csr_csc(t, prec)
    same(got[0], want[0], "CSR")
    same(got[1], want[1], "CSC")
