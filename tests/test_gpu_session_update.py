"""Session updates on the device (include/poismf_hip.h section 2b): Session.add merges new counts into the resident CSR and CSC,
Session.half_sweep_rows refits listed rows, Session.update does both.  Every assertion is bit equality: the merged matrix against SciPy's
X + D, the merged session against a fresh session on X + D, a listed row against the same row of a full half-sweep (a row's arithmetic
depends on its length class only, tests/test_gpu_invariance.py).  Counts are integer-valued unless a test says otherwise, so sums are exact
in any order.  Needs an MI355X."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.test_gpu_invariance import CASES, DIMB, SEGMENT_LENGTHS, a_half, checker_a_half, params_for, problem

pytestmark = pytest.mark.gpu
KNOBS_SET = [v for v in os.environ if v.startswith("POISMF_HIP_")]


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def session_of(X, k, prec, how="coo", **kw):
    """a session on the SciPy matrix X: built on the device from its triplets, or from the host CSR / CSC"""
    if how == "coo":
        return api.Session.from_coo(X.tocoo(), k, prec, **kw)
    csr, csc = harness.process_data(X.tocoo(), prec)
    return api.Session(csr, csc, X.shape[0], X.shape[1], k, prec, **kw)


def total(X, D, prec):
    """X + D as the session must hold it: duplicates inside each summed first, then one addition per cell, all in the session's precision"""
    dt = H.dtype_of(prec)
    Xs, Ds = X.astype(dt).tocsr(), D.astype(dt).tocsr()
    Xs.sum_duplicates(); Ds.sum_duplicates()
    S = (Xs + Ds).tocsr()
    S.sort_indices()
    return S


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_matrix(got, want, what):
    val, ind, ptr = got
    assert np.array_equal(ptr.astype(np.int64), want.indptr.astype(np.int64)), f"{what}: row pointers differ"
    assert np.array_equal(ind.astype(np.int64), want.indices.astype(np.int64)), f"{what}: indices differ"
    assert val.dtype == want.data.dtype and np.array_equal(bits(val), bits(want.data)), f"{what}: values differ in bits"


def holds(s, S, what):
    """both orientations of session s are the SciPy matrix S, and the counts agree"""
    Sc = S.tocsc()
    Sc.sort_indices()
    same_matrix(s.matrix(1), S, what + " (CSR)")
    same_matrix(s.matrix(0), Sc, what + " (CSC)")
    assert s.nnz(0) == s.nnz(1) == S.nnz


def same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} entries differ in bits"


# ---- 1. the merged matrix against SciPy ----------------------------------------------------------------------------------------------
DIMA1, DIMB1, HOT, NEVER = 400, 6000, 3000, 5999
SPECIAL = {10: 0, 20: 1, 30: 63, 31: 64, 32: 65, 100: 1024, 101: 1025, 200: 5000}   # row -> stored cells


def big_problem(integer=True, seed=3):
    """X (400 x 6000): row lengths 0, 1, 63, 64, 65, 1024, 1025 and 5000 between random short rows; column HOT stored in nearly every row (a
    long CSC row); column NEVER stored nowhere.  D holds every situation the merge distinguishes (the comments below)."""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(DIMB1), [HOT, NEVER])
    rows, cols = [], []
    stored = {}
    for r in range(DIMA1):
        n = SPECIAL.get(r, int(rng.integers(2, 40)))
        pool = free[(free >= 100) & (free < 5900)] if r == 31 else free
        if n == 0:
            c = np.zeros(0, np.int64)
        elif n == 1:
            c = rng.choice(pool, size=1)
        else:
            c = np.concatenate([rng.choice(pool, size=n - 1, replace=False), [HOT]])
        stored[r] = np.sort(c)
        rows.append(np.full(len(c), r)); cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    X = sp.coo_matrix((1.0 + np.floor(rng.gamma(1.0, 1.0, len(row))), (row, col)), shape=(DIMA1, DIMB1))

    def fresh_cols(r, n):
        return rng.choice(np.setdiff1d(free, stored[r]), size=n, replace=False)

    d = []
    d += [(10, c) for c in fresh_cols(10, 50)] + [(10, HOT)]            # an empty row filled, the hot column among its cells
    d += [(30, c) for c in stored[30][::6]]                             # a row hit on stored cells only: its length stays
    d += [(31, 5), (31, 5990)]                                          # before a row's first entry, behind its last
    d += [(0, fresh_cols(0, 1)[0]), (0, stored[0][0])]                  # the first row
    d += [(DIMA1 - 1, fresh_cols(DIMA1 - 1, 1)[0]), (DIMA1 - 1, stored[DIMA1 - 1][-1])]   # the last row
    d += [(100, c) for c in fresh_cols(100, 7)] + [(100, stored[100][500])]              # two adjacent touched rows: 100 and 101 ...
    d += [(101, c) for c in fresh_cols(101, 3000)] + [(101, c) for c in stored[101][::100]]   # ... the 1025-row with 3000 new cells
    d += [(200, fresh_cols(200, 1)[0])]                                 # the 5000-row with one new cell
    d += [(50, NEVER), (51, NEVER)]                                     # a column never stored before
    d += [(60, HOT), (61, HOT), (62, HOT)]                              # the hot column, hit
    d = np.array(d, dtype=np.int64)
    if integer:
        d = np.concatenate([d, d[::7], d[::7], d[:3]])                  # triplets repeated inside D
        dval = 1.0 + np.floor(rng.gamma(1.0, 1.0, len(d)))
    else:
        # at most one triplet per cell, non-integer values: a stored cell gets ONE rounded addition
        X = sp.coo_matrix((rng.uniform(0.1, 9.0, X.nnz), (X.row, X.col)), shape=X.shape)
        dval = rng.uniform(0.1, 9.0, len(d))
    order = rng.permutation(len(d))
    D = sp.coo_matrix((dval[order], (d[order, 0], d[order, 1])), shape=X.shape)
    return X, D


@pytest.mark.parametrize("how", ["coo", "host"])
def test_merged_matrix_is_scipy_s_sum(prec, how):
    X, D = big_problem()
    S = total(X, D, prec)
    s = session_of(X, 8, prec, how)
    try:
        holds(s, total(X, sp.coo_matrix(X.shape), prec), "before the update")
        fresh = s.add(D)
        assert fresh == S.nnz - X.tocsr().nnz
        holds(s, S, f"after the update ({how})")
    finally:
        s.close()


def test_a_stored_cell_gets_one_rounded_addition(prec):
    X, D = big_problem(integer=False)
    S = total(X, D, prec)
    s = session_of(X, 8, prec)
    try:
        assert s.add(D) == S.nnz - X.nnz
        holds(s, S, "non-integer values")
    finally:
        s.close()


# ---- 2. edges of the decomposition ---------------------------------------------------------------------------------------------------
def small_counts(dimA, dimB, n, seed):
    rng = np.random.default_rng(seed)
    return sp.coo_matrix((1.0 + np.floor(rng.gamma(1.0, 1.0, n)), (rng.integers(0, dimA, n), rng.integers(0, dimB, n))), shape=(dimA, dimB))


def test_edges_of_the_decomposition(prec):
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 400, 1)
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    stored = Xs.tocoo()
    absent = np.argwhere(Xs.toarray() == 0)
    one = lambda r, c, v=2.0: sp.coo_matrix(([v], ([r], [c])), shape=X.shape)
    every_row = sp.coo_matrix((np.full(dimA, 3.0), (np.arange(dimA), (7 * np.arange(dimA) + 1) % dimB)), shape=X.shape)
    updates = {
        "one new cell": one(*absent[11]),
        "one stored cell": one(stored.row[5], stored.col[5]),
        "every row": every_row,
        "larger than X": small_counts(dimA, dimB, 3000, 2),
    }
    for what, D in updates.items():
        s = session_of(X, 4, prec)
        try:
            S = total(X, D, prec)
            assert s.add(D) == S.nnz - Xs.nnz, what
            holds(s, S, what)
        finally:
            s.close()


def test_three_updates_equal_one_fresh_session(prec):
    dimA, dimB = 57, 83
    X, Ds = small_counts(dimA, dimB, 400, 1), [small_counts(dimA, dimB, n, 10 + n) for n in (30, 500, 1)]
    s = session_of(X, 4, prec)
    T = X
    try:
        for D in Ds:
            before = total(T, sp.coo_matrix(X.shape), prec).nnz
            T = (T.tocsr() + D.tocsr()).tocoo()
            assert s.add(D) == total(T, sp.coo_matrix(X.shape), prec).nnz - before
        f = session_of(T, 4, prec)
        try:
            for which in (0, 1):
                for got, want in zip(s.matrix(which), f.matrix(which)):
                    assert got.dtype == want.dtype and np.array_equal(got, want)
        finally:
            f.close()
    finally:
        s.close()


def test_an_update_without_a_new_cell_keeps_pointers_and_indices(prec):
    X = small_counts(57, 83, 400, 1)
    s = session_of(X, 4, prec)
    try:
        before = [s.matrix(w) for w in (0, 1)]
        pick = X.tocsr().tocoo()
        D = sp.coo_matrix((np.full(40, 2.0), (pick.row[::7][:40], pick.col[::7][:40])), shape=X.shape)
        assert s.add(D) == 0
        for w in (0, 1):
            val, ind, ptr = s.matrix(w)
            assert np.array_equal(ind, before[w][1]) and np.array_equal(ptr, before[w][2])
            assert not np.array_equal(val, before[w][0])
        holds(s, total(X, D, prec), "hits only")
    finally:
        s.close()


# ---- 3. the merged session behaves as a fresh one -------------------------------------------------------------------------------------
def two_sided(seed=5, dimA=310, dimB=190):
    rng = np.random.default_rng(seed)
    p = (np.arange(dimB) + 1.0) ** -0.8
    n = 4000
    X = sp.coo_matrix((1.0 + np.floor(rng.gamma(1.0, 1.0, n)), (rng.integers(0, dimA, n), rng.choice(dimB, size=n, p=p / p.sum()))), shape=(dimA, dimB))
    m = 600
    D = sp.coo_matrix((1.0 + np.floor(rng.gamma(1.0, 1.0, m)), (rng.integers(0, dimA // 3, m), rng.choice(dimB, size=m, p=p / p.sum()))), shape=(dimA, dimB))
    return X, D


@pytest.mark.parametrize("case", ["pg-f32-k50", "cg-f64-k50", "tncg-f64-k50"])
def test_the_merged_session_is_a_fresh_session(case):
    method, prec, k, maxupd, _ = CASES[case]
    X, D = two_sided()
    S = total(X, D, prec)
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    users = np.arange(0, dimA, 3)
    new_rows = small_counts(12, dimB, 150, 21).tocsr()
    s, f = session_of(X, k, prec), session_of(S, k, prec)
    try:
        p, cd = params_for(s, case)
        for x in (s, f):
            assert x.set_segments(1, 4) == 4
        # everything add() must refresh or leave alone has been used once before it: the row pointers exclude_seen keeps, and the guest
        s.set_factors(A0, B0)
        s.topn_batch(users, 10, exclude_seen=True, output_score=True)
        s.topn_new(new_rows, p, 3, top_n=5, output_score=True)
        assert s.add(D) == S.nnz - total(X, sp.coo_matrix(X.shape), prec).nnz
        assert [s.segment_rows(1, j) for j in range(4)] == [f.segment_rows(1, j) for j in range(4)]
        out = []
        for x in (s, f):
            x.set_factors(A0, B0)
            x.half_sweep(0, p, 1e-7, cd)
            B1 = x.get_factors()[1]
            x.half_sweep(1, p, 1e-7, cd)
            A, B = x.get_factors()
            out.append(dict(A=A, B=B, B1=B1, llk=x.llk(), top=x.topn_batch(users, 10, exclude_seen=True, output_score=True),
                            new=x.topn_new(new_rows, p, 3, top_n=5, output_score=True, return_factors=True), plan=(x.plan(0), x.plan(1))))
        m, w = out
        same_bits(m["B"], w["B"], "B after the B half")
        same_bits(m["A"], w["A"], "A after the A half")
        assert m["llk"] == w["llk"] and np.isfinite(m["llk"])
        assert np.array_equal(m["top"][0], w["top"][0])
        same_bits(m["top"][1], w["top"][1], "top-N scores")
        assert np.array_equal(m["new"][0], w["new"][0])
        same_bits(m["new"][1], w["new"][1], "scores of the new rows")
        same_bits(m["new"][2], w["new"][2], "factors of the new rows")
        assert m["plan"] == w["plan"]
        seen = S.toarray() > 0
        assert not seen[users[:, None], m["top"][0].astype(np.int64)].any()   # exclude_seen knows the new cells
        if case == "pg-f32-k50":
            # equal bits are not equal wrong answers: the A half on X + D against the checker, by tests/test_gpu_parity.py compare()'s PG rule
            Ss = S.astype(H.dtype_of(prec))
            csr = (Ss.data, Ss.indices.astype(np.uint64), Ss.indptr.astype(np.uint64))
            Ar, _, _ = checker_a_half(case, csr, A0, m["B1"])
            err = H.scaled_err(m["A"], Ar)
            print(f"{case}: A half of the merged session vs the checker on X + D: {err:.3g}")
            assert np.isfinite(m["A"]).all() and err <= 1e-5
    finally:
        s.close(); f.close()


# ---- 4. refusals leave the session as it was ------------------------------------------------------------------------------------------
def unchanged(s, before):
    for w in (0, 1):
        for got, want in zip(s.matrix(w), before[w]):
            assert np.array_equal(got, want)


def test_refusals_leave_the_session_as_it_was(prec):
    dt = H.dtype_of(prec)
    X = small_counts(57, 83, 400, 1)
    D = small_counts(57, 83, 50, 2)
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)

    def raw_add(s, row, col, val):
        n = C.c_size_t(99)
        row, col, val = u64(row), u64(col), np.ascontiguousarray(val, dtype=dt)
        return s.lib.poismf_hip_session_add_coo(s.h, api._ptr(row), api._ptr(col), api._ptr(val), len(val), C.byref(n))

    s = session_of(X, 4, prec)
    try:
        before = [s.matrix(w) for w in (0, 1)]
        assert raw_add(s, [3, 57], [3, 0], [1.0, 1.0]) == 3        # an index outside, past the binding's own check
        assert raw_add(s, [3, 4], [3, 83], [1.0, 1.0]) == 3
        for v in (0.0, -1.0, np.nan, np.inf):
            assert raw_add(s, [3, 4], [3, 5], [1.0, v]) == 4
        with pytest.raises(ValueError):
            s.add(sp.coo_matrix(([1.0], ([0], [0])), shape=(58, 83)))
        unchanged(s, before)
    finally:
        s.close()

    csr, csc = harness.process_data(X.tocoo(), prec)
    s = api.Session(csr, csc, 57, 83, 4, prec, shardA=(0, 30))     # a sharded session
    try:
        before = [s.matrix(w) for w in (0, 1)]
        with pytest.raises(ValueError):
            s.add(D)
        unchanged(s, before)
    finally:
        s.close()

    for side in (0, 1):                                            # one descending row in the host CSC / CSR
        cs = [[a.copy() for a in csc], [a.copy() for a in csr]]
        val, ind, ptr = cs[side]
        r = int(np.flatnonzero(np.diff(ptr.astype(np.int64)) >= 2)[0])
        p0 = int(ptr[r])
        ind[[p0, p0 + 1]] = ind[[p0 + 1, p0]]
        val[[p0, p0 + 1]] = val[[p0 + 1, p0]]
        s = api.Session(cs[1], cs[0], 57, 83, 4, prec)
        try:
            before = [s.matrix(w) for w in (0, 1)]
            with pytest.raises(ValueError):
                s.add(D)
            unchanged(s, before)
        finally:
            s.close()


# ---- 5. listed rows -------------------------------------------------------------------------------------------------------------------
def engines(plan):
    """(register instances may differ where a bin rides with another: compared without S, as tests/test_gpu_invariance.py does)"""
    return {re.sub(r"S=\d+", "S=*", name) for name, _ in plan}


@pytest.mark.parametrize("case", ["pg-f32-k50", "cg-f64-k50", "tncg-f64-k100", "tncg-f32-k20"])
def test_listed_rows_get_the_full_half_sweep_s_bits(case):
    method, prec, k, maxupd, _ = CASES[case]
    csr, csc, A0, B0 = problem(case, lengths=SEGMENT_LENGTHS)
    dimA = A0.shape[0]
    lengths = np.diff(csr[2].astype(np.int64))
    rng = np.random.default_rng(17)
    third = rng.permutation(np.arange(0, dimA, 3))
    lists = {
        "every third row": third,
        "the complement": rng.permutation(np.setdiff1d(np.arange(dimA), third)),
        "all rows": rng.permutation(dimA),
        "the longest row": np.array([int(np.argmax(lengths))]),
        "the empty row": np.array([int(np.flatnonzero(lengths == 0)[0])]),
        "no row": np.zeros(0, np.int64),
    }
    s = api.Session(csr, csc, dimA, DIMB, k, prec)
    try:
        full, n_full = a_half(s, case, A0, B0)
        base_engines = engines(s.plan(1))
        p, cd = params_for(s, case)
        counts = {}
        for what, rows in lists.items():
            s.set_factors(A0, B0)
            counts[what] = s.half_sweep_rows(1, rows, p, 1e-7, cd, want_unchanged=method == "tncg")
            A = s.get_factors()[0]
            listed = np.zeros(dimA, bool)
            listed[rows] = True
            same_bits(A[listed], full[listed], f"{case}, {what}: listed rows against the full half-sweep")
            same_bits(A[~listed], A0[~listed], f"{case}, {what}: unlisted rows against the start")
            if len(rows) and not KNOBS_SET:
                assert engines(s.plan(1)) <= base_engines, (what, sorted(engines(s.plan(1)) - base_engines))
                assert sum(n for _, n in s.plan(1)) == len(rows)
        if method == "tncg":
            assert counts["every third row"] + counts["the complement"] == n_full == counts["all rows"]
            assert counts["no row"] == 0
    finally:
        s.close()


@pytest.mark.parametrize("case", ["pg-f32-k50", "cg-f64-k50"])
def test_listed_rows_of_the_b_half(case):
    method, prec, k, maxupd, _ = CASES[case]
    X, _ = two_sided()
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    s = session_of(X, k, prec)
    try:
        p, cd = params_for(s, case)
        s.set_factors(A0, B0)
        s.half_sweep(0, p, 1e-7, cd)
        full = s.get_factors()[1]
        rows = np.random.default_rng(2).permutation(np.arange(1, dimB, 2))
        s.set_factors(A0, B0)
        s.half_sweep_rows(0, rows, p, 1e-7, cd)
        A, B = s.get_factors()
        listed = np.zeros(dimB, bool)
        listed[rows] = True
        same_bits(B[listed], full[listed], "listed rows of B")
        same_bits(B[~listed], B0[~listed], "unlisted rows of B")
        same_bits(A, A0, "A")
    finally:
        s.close()


def test_the_padded_copy_follows_a_call_over_listed_rows():
    """k = 50 fp32: the session gathers from line-padded copies of the factors.  After a call over listed rows of A -- with the copy of A stale
    (factors just set) and with it fresh (a full A half before) -- a full B half must read the A that get_factors shows."""
    case = "pg-f32-k50"
    method, prec, k, maxupd, _ = CASES[case]
    X, _ = two_sided()
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    rows = np.random.default_rng(4).permutation(np.arange(0, dimA, 4))
    s, f = session_of(X, k, prec), session_of(X, k, prec)
    try:
        p, cd = params_for(s, case)
        for fresh_copy in (False, True):
            s.set_factors(A0, B0)
            if fresh_copy:
                s.half_sweep(1, p, 1e-7, cd)
            s.half_sweep_rows(1, rows, p, 1e-7, cd)
            A, B = s.get_factors()
            same_bits(B, B0, "B")
            assert not np.array_equal(A[rows], A0[rows])
            s.half_sweep(0, p, 1e-7, cd)
            f.set_factors(A, B0)
            f.half_sweep(0, p, 1e-7, cd)
            same_bits(s.get_factors()[1], f.get_factors()[1], f"the B half after listed rows of A (copy of A fresh before: {fresh_copy})")
    finally:
        s.close(); f.close()


# ---- 6. update ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pg-f32-k50", "tncg-f64-k50"])
def test_update_is_add_and_two_calls_over_listed_rows(case):
    method, prec, k, maxupd, _ = CASES[case]
    X, D = two_sided()
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    users, items = np.unique(D.row), np.unique(D.col)
    s, f = session_of(X, k, prec), session_of(X, k, prec)
    try:
        p, _ = params_for(s, case)
        s.set_factors(A0, B0); f.set_factors(A0, B0)
        got = s.update(D, p, 1e-7)
        assert np.array_equal(got[0], users) and np.array_equal(got[1], items)
        f.add(D)
        step = f.real(1e-7)
        cd = f.cnst_div(p.l2_reg, step)
        f.half_sweep_rows(1, users, p, step, cd)
        f.half_sweep_rows(0, items, p, step, cd)
        (A, B), (Af, Bf) = s.get_factors(), f.get_factors()
        same_bits(A, Af, "A"); same_bits(B, Bf, "B")
        untouched_users = np.setdiff1d(np.arange(dimA), users)
        same_bits(A[untouched_users], A0[untouched_users], "rows of A the update does not name")
        assert not np.array_equal(A[users], A0[users])
    finally:
        s.close(); f.close()
