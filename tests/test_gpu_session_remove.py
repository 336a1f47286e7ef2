"""Counts taken back from a resident session on the device (include/poismf_hip.h section 2c): Session.subtract, remove, forget and retract.
Every assertion is bit equality, against an expectation built in numpy / SciPy that holds no GPU code (expected(), below): duplicates of D
summed in the model's dtype, then nv = x - d in that dtype, the cell kept if and only if nv > 0, indices sorted.  Counts are integer-valued
unless a test says otherwise, so sums are exact in any order.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.test_gpu_invariance import CASES, params_for
from tests.test_gpu_session_update import (DIMA1, DIMB1, HOT, NEVER, big_problem, holds, same_bits, session_of, small_counts, total,
                                           two_sided)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def cells(rows, cols, vals, shape, dt=np.float64):
    return sp.coo_matrix((np.asarray(vals, dtype=dt), (np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64))), shape=shape)


def expected(X, D, prec, remove=False):
    """(X - D as the session must hold it, cells that leave, listed cells X does not store).  X's cells are distinct or integer-valued; D's
    triplets are summed per cell in the session's precision, a stored cell gets ONE subtraction in that precision and stays iff the result
    is > 0; with remove every listed stored cell leaves whatever it holds."""
    dt = H.dtype_of(prec)
    Xs, Ds = X.astype(dt).tocsr(), sp.coo_matrix(D).astype(dt).tocsr()
    Xs.sum_duplicates(); Ds.sum_duplicates()
    x, d = Xs.toarray(), Ds.toarray()
    stored = np.zeros(x.shape, bool)
    stored[Xs.nonzero()] = True
    assert (x[stored] > 0).all()
    listed = np.zeros(x.shape, bool)
    Dc = sp.coo_matrix(D)
    listed[Dc.row, Dc.col] = True
    nv = x - d
    assert x.dtype == d.dtype == nv.dtype == dt
    gone = stored & listed & (True if remove else ~(nv > 0))
    E = sp.csr_matrix(np.where(stored & ~gone, np.where(listed, nv, x), dt(0)).astype(dt))
    E.sort_indices()
    assert E.nnz == int((stored & ~gone).sum())
    return E, int(gone.sum()), int((listed & ~stored).sum())


def as_scipy(m, shape, csc=False):
    val, ind, ptr = m
    make = sp.csc_matrix if csc else sp.csr_matrix
    return make((val, ind.astype(np.int64), ptr.astype(np.int64)), shape=shape)


def snapshot(s):
    return [s.matrix(w) for w in (0, 1)]


def unchanged(s, before):
    for w in (0, 1):
        for got, want in zip(s.matrix(w), before[w]):
            assert got.dtype == want.dtype and np.array_equal(got, want)


# ---- 1. against SciPy -----------------------------------------------------------------------------------------------------------------
def removal_list(S, rng):
    """(row, col, value) triplets over the stored matrix S = X + D of big_problem(), one group per situation the compaction distinguishes.
    Cells of `out` leave under subtract (their whole value is listed, some in two triplets); cells of `dec` lose 1 of a value >= 2 and stay."""
    S = S.tocsr()
    ptr, ind = S.indptr.astype(np.int64), S.indices.astype(np.int64)
    row = lambda r: ind[ptr[r]:ptr[r + 1]]
    out = []
    out += [(10, c) for c in row(10)]                                    # a row emptied completely (51 cells) ...
    out += [(20, c) for c in row(20)]                                    # ... and a row of one cell
    out += [(30, row(30)[0])]                                            # a row losing its first entry only
    out += [(31, row(31)[-1])]                                           # its last only
    out += [(32, row(32)[30])]                                           # one in the middle
    out += [(0, row(0)[1]), (DIMA1 - 1, row(DIMA1 - 1)[1])]              # the first row and the last row
    out += [(100, c) for c in row(100)[[0, 200, 201, 700, -1]]]          # two adjacent touched rows: 100 and 101 ...
    out += [(101, c) for c in row(101)[::4][:1000]]                      # ... the 1025-row (4025 cells by now) losing 1000
    edge = (ptr[200] // 4096 + 1) * 4096 - ptr[200]                      # the 5000-row straddles a chunk of 4096 resident entries:
    assert 0 < edge < len(row(200)) - 1
    out += [(200, row(200)[j]) for j in sorted({edge - 1, edge, 4095, 4096})]   # one cell on each side of the cut, and of its own entry 4096
    hot_rows = np.flatnonzero(np.asarray((S[:, HOT] != 0).todense()).ravel())
    out += [(r, HOT) for r in hot_rows if r != 77 and (r, HOT) not in set(out)]   # the hot column losing all but one cell
    out += [(r, NEVER) for r in (50, 51)]                                # a column emptied
    out = list(dict.fromkeys((int(r), int(c)) for r, c in out))
    taken = set(out)
    coo = S.tocoo()
    rich = [(int(r), int(c)) for r, c, v in zip(coo.row, coo.col, coo.data) if v >= 2 and (int(r), int(c)) not in taken]
    dec = [rich[i] for i in rng.choice(len(rich), size=200, replace=False)]
    trip = []
    for i, (r, c) in enumerate(out):
        v = float(S[r, c])
        trip += [(r, c, 1.0), (r, c, v - 1.0)] if i % 5 == 0 and v >= 2 else [(r, c, v)]   # triplets repeated inside D
    trip += [(r, c, 1.0) for r, c in dec]
    trip = [trip[i] for i in rng.permutation(len(trip))]
    r, c, v = zip(*trip)
    return cells(r, c, v, S.shape), out, dec


@pytest.mark.parametrize("how", ["coo", "host"])
def test_the_smaller_matrix_is_scipy_s(prec, how):
    X, D = big_problem()
    S = total(X, D, prec)
    R, out, dec = removal_list(S, np.random.default_rng(11))
    assert len(R.data) > len(out) + len(dec)   # some cells are listed twice
    for remove in (False, True):
        E, n_gone, n_absent = expected(S, R, prec, remove)
        assert n_absent == 0 and n_gone == (len(out) + len(dec) if remove else len(out))
        lens = np.diff(E.indptr)
        assert lens[10] == 0 and lens[20] == 0 and E.tocsc()[:, NEVER].nnz == 0 and E.tocsc()[:, HOT].nnz == 1
        s = session_of(X, 8, prec, how)
        try:
            s.add(D)
            holds(s, S, "before the removal")
            got = s.remove(R, missing="raise") if remove else s.subtract(R)
            assert got == n_gone
            holds(s, E, f"after {'remove' if remove else 'subtract'} ({how})")
        finally:
            s.close()


# ---- 2. round trip --------------------------------------------------------------------------------------------------------------------
def test_add_then_subtract_gives_x_back(prec):
    X, D = big_problem()
    X0 = total(X, sp.coo_matrix(X.shape), prec)
    created = total(X, D, prec).nnz - X0.nnz
    assert created > 3000
    s = session_of(X, 8, prec)
    try:
        assert s.add(D) == created
        assert s.subtract(D) == created        # every cell D created is gone, every other cell has its count back
        holds(s, X0, "add(D) then subtract(D)")
    finally:
        s.close()


# ---- 3. the sign rule -----------------------------------------------------------------------------------------------------------------
def test_the_sign_rule(prec):
    dt = H.dtype_of(prec)
    dimA, dimB, n = 57, 83, 900
    rng = np.random.default_rng(6)
    where = rng.permutation(dimA * dimB)[:n]
    r, c = where // dimB, where % dimB
    x = rng.uniform(0.1, 9.0, n).astype(dt)
    d = rng.uniform(0.1, 9.0, n).astype(dt)        # non-integer values, one triplet per cell: one rounded subtraction, either sign
    zero, below, ulp = slice(0, 100), slice(100, 200), slice(200, 300)
    d[zero] = x[zero]                              # to exactly 0: removed
    d[below] = x[below] * dt(2)                  # below 0: removed
    d[ulp] = x[ulp]
    x[ulp] = np.nextafter(x[ulp], dt(np.inf))      # to the smallest positive difference at that magnitude: kept
    assert x.dtype == dt and d.dtype == dt
    listed = rng.permutation(n)[:700]
    listed = np.union1d(listed, np.arange(300))
    X, D = cells(r, c, x, (dimA, dimB), dt), cells(r[listed], c[listed], d[listed], (dimA, dimB), dt)
    E, n_gone, n_absent = expected(X, D, prec)
    dense = E.toarray()
    assert n_absent == 0 and not dense[r[zero], c[zero]].any() and not dense[r[below], c[below]].any()
    same_bits(dense[r[ulp], c[ulp]], x[ulp] - d[ulp], "the expectation keeps one ulp")
    assert (dense[r[ulp], c[ulp]] > 0).all() and 200 < n_gone < len(listed)
    s = session_of(X, 4, prec)
    try:
        assert s.subtract(D) == n_gone
        holds(s, E, "the sign rule")
        csr, csc = as_scipy(s.matrix(1), X.shape), as_scipy(s.matrix(0), X.shape, csc=True)
        assert (csr.data > 0).all() and (csc.data > 0).all()
        assert (csr != csc.tocsr()).nnz == 0 and np.array_equal(csr.toarray() != 0, csc.toarray() != 0)   # both orientations agree
    finally:
        s.close()


# ---- 4. edges on 57 x 83 ----------------------------------------------------------------------------------------------------------------
def test_edges_of_the_compaction(prec):
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 400, 1)
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    stored = Xs.tocoo()
    first = Xs.indptr[:-1][np.diff(Xs.indptr) > 0]
    lists = {
        "one stored cell, to zero": (cells([stored.row[5]], [stored.col[5]], [stored.data[5]], X.shape), "raise"),
        "one stored cell, kept": (cells([stored.row[stored.data >= 2][0]], [stored.col[stored.data >= 2][0]], [1.0], X.shape), "raise"),
        "every row": (cells(stored.row[first], stored.col[first], np.ones(len(first)), X.shape), "raise"),
        "larger than X": (small_counts(dimA, dimB, 3000, 2), "ignore"),
    }
    assert len(first) == dimA
    for what, (D, missing) in lists.items():
        for remove in (False, True):
            E, n_gone, n_absent = expected(Xs, D, prec, remove)
            assert (n_absent > 1000) == (what == "larger than X")
            s = session_of(X, 4, prec)
            try:
                assert (s.remove(D, missing=missing) if remove else s.subtract(D, missing=missing)) == n_gone, what
                holds(s, E, what)
            finally:
                s.close()
    # the list larger than X: the cells that go are the stored ones among the listed
    R = small_counts(dimA, dimB, 3000, 2).tocsr()
    assert expected(Xs, R, prec, True)[1] == (R.astype(bool).multiply(Xs.astype(bool))).nnz


def test_an_emptied_matrix_takes_new_counts(prec):
    X = small_counts(57, 83, 400, 1)
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    D = small_counts(57, 83, 120, 8)
    s = session_of(X, 4, prec)
    try:
        assert s.remove(Xs) == Xs.nnz
        assert s.nnz(0) == 0 and s.nnz(1) == 0
        holds(s, sp.csr_matrix(X.shape, dtype=H.dtype_of(prec)), "every stored cell removed")
        assert s.remove(Xs) == 0 and s.forget(1, np.arange(57)) == 0
        Ds = total(D, sp.coo_matrix(X.shape), prec)
        assert s.add(D) == Ds.nnz
        holds(s, Ds, "add on the emptied matrix")
    finally:
        s.close()


def test_three_removals_equal_one_fresh_session(prec):
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 900, 1)
    T = total(X, sp.coo_matrix(X.shape), prec)
    s = session_of(X, 4, prec)
    try:
        for i, n in enumerate((30, 500, 1)):
            D = small_counts(dimA, dimB, n, 10 + n)
            remove = i == 1
            T, n_gone, _ = expected(T, D, prec, remove)
            assert (s.remove(D) if remove else s.subtract(D, missing="ignore")) == n_gone
        f = session_of(T, 4, prec)
        try:
            for which in (0, 1):
                for got, want in zip(s.matrix(which), f.matrix(which)):
                    assert got.dtype == want.dtype and np.array_equal(got, want)
        finally:
            f.close()
    finally:
        s.close()


# ---- 5. strict, and refusals leave the session as it was -------------------------------------------------------------------------------
def test_refusals_leave_the_session_as_it_was(prec):
    dt = H.dtype_of(prec)
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 400, 1)
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    stored = Xs.tocoo()
    ar, ac = np.argwhere(Xs.toarray() == 0)[17]
    many = cells(np.append(stored.row[::2], ar), np.append(stored.col[::2], ac), np.ones(len(stored.row[::2]) + 1), X.shape)   # one absent cell among 150 stored
    good = cells(stored.row[::2], stored.col[::2], np.ones(len(stored.row[::2])), X.shape)
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)

    def raw_sub(s, row, col, val, strict):
        gone, absent = C.c_size_t(99), C.c_size_t(99)
        row, col = u64(row), u64(col)
        val = None if val is None else np.ascontiguousarray(val, dtype=dt)
        rc = s.lib.poismf_hip_session_sub_coo(s.h, api._ptr(row), api._ptr(col), None if val is None else api._ptr(val), len(row), strict,
                                              C.byref(gone), C.byref(absent))
        return rc, gone.value, absent.value

    def raw_rows(s, which, rows):
        gone = C.c_size_t(99)
        rows = u64(rows)
        return s.lib.poismf_hip_session_remove_rows(s.h, which, api._ptr(rows), len(rows), C.byref(gone))

    s = session_of(X, 4, prec)
    try:
        before = snapshot(s)
        for method in (s.subtract, lambda D: s.remove(D, missing="raise")):
            with pytest.raises(ValueError):
                method(many)
            unchanged(s, before)
        assert raw_sub(s, many.row, many.col, many.data, 1) == (6, 0, 1)
        assert raw_sub(s, many.row, many.col, None, 1) == (6, 0, 1)
        assert raw_sub(s, [3, 57], [3, 0], [1.0, 1.0], 0)[0] == 3        # an index outside, past the binding's own check
        assert raw_sub(s, [3, 4], [3, 83], None, 0)[0] == 3
        for v in (0.0, -1.0, np.nan, np.inf):
            assert raw_sub(s, [3, 4], [3, 5], [1.0, v], 0)[0] == 4
        assert raw_rows(s, 1, [3, 57]) == 3 and raw_rows(s, 0, [83]) == 3 and raw_rows(s, 1, [5, 9, 5]) == 3
        assert raw_sub(s, [], [], None, 1) == (0, 0, 0) and raw_rows(s, 1, []) == 0
        unchanged(s, before)
    finally:
        s.close()

    csr, csc = harness.process_data(X.tocoo(), prec)
    s = api.Session(csr, csc, dimA, dimB, 4, prec, shardA=(0, 30))     # a session that holds a shard
    try:
        before = snapshot(s)
        for call in (lambda: s.subtract(good), lambda: s.subtract(many), lambda: s.remove(good), lambda: s.forget(1, [3]), lambda: s.forget(0, [3])):
            with pytest.raises(ValueError):
                call()
        assert raw_sub(s, good.row, good.col, good.data, 0)[0] == 5 and raw_rows(s, 1, [3]) == 5
        unchanged(s, before)
    finally:
        s.close()

    for side in (0, 1):                                                # one descending row in the host CSC / CSR
        cs = [[a.copy() for a in csc], [a.copy() for a in csr]]
        val, ind, ptr = cs[side]
        r = int(np.flatnonzero(np.diff(ptr.astype(np.int64)) >= 2)[0])
        p0 = int(ptr[r])
        ind[[p0, p0 + 1]] = ind[[p0 + 1, p0]]
        val[[p0, p0 + 1]] = val[[p0 + 1, p0]]
        s = api.Session(cs[1], cs[0], dimA, dimB, 4, prec)
        try:
            before = snapshot(s)
            for call in (lambda: s.subtract(good), lambda: s.subtract(many), lambda: s.remove(good), lambda: s.forget(1, [3]), lambda: s.forget(0, [3])):
                with pytest.raises(ValueError):
                    call()
            assert raw_sub(s, good.row, good.col, None, 1)[0] == 5 and raw_rows(s, 0, [3]) == 5
            unchanged(s, before)
        finally:
            s.close()


# ---- 6. forget ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["coo", "host"])
def test_forget(prec, how):
    X, _ = big_problem()
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    col_len = np.diff(Xs.tocsc().indptr)
    short = int(np.flatnonzero((col_len >= 1) & (col_len <= 3))[0])
    assert col_len[NEVER] == 0 and col_len[HOT] > 390
    users = np.array([200, 10, 0, 101, DIMA1 - 1, 20])                 # the 5000-row, an empty row, the first row, the 1025-row, the last row, a 1-row
    items = np.array([short, NEVER, HOT])
    s = session_of(X, 8, prec, how)
    try:
        E = Xs.tolil()
        E[users, :] = 0
        E = E.tocsr()
        E.eliminate_zeros(); E.sort_indices()
        assert s.forget(1, users) == Xs.nnz - E.nnz == int(np.diff(Xs.indptr)[users].sum())
        holds(s, E, "forget(1, users)")
        assert s.forget(1, users) == 0
        holds(s, E, "forget(1, users) again")
        E2 = E.tocsc()
        gone = int(np.diff(E2.indptr)[items].sum())
        E2 = E2.tolil()
        E2[:, items] = 0
        E2 = E2.tocsr()
        E2.eliminate_zeros(); E2.sort_indices()
        assert s.forget(0, items) == gone == E.nnz - E2.nnz and gone > 380
        holds(s, E2, "forget(0, items)")
        before = snapshot(s)
        assert s.forget(0, items) == 0 and s.forget(0, [NEVER]) == 0
        unchanged(s, before)
    finally:
        s.close()


# ---- 7. the rest of the session sees it ------------------------------------------------------------------------------------------------
def two_sided_removal(prec, seed=13):
    """X of tests/test_gpu_session_update.py's two_sided(), the counts subtracted from it (600 stored cells of the first third of the users lose
    1: those that held 1 leave), the users and the item forgotten after that, and the expectation"""
    X, _ = two_sided()
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    rng = np.random.default_rng(seed)
    coo = Xs.tocoo()
    pool = np.flatnonzero(coo.row < X.shape[0] // 3)
    pick = rng.choice(pool, size=600, replace=False)
    D = cells(coo.row[pick], coo.col[pick], np.ones(600), X.shape)
    users, item = np.array([5, 250, 77]), np.array([0])                # (item 0 is the most popular one: a long CSC row)
    E, n_gone, _ = expected(Xs, D, prec)
    assert 100 < n_gone < 500
    E = E.tolil()
    E[users, :] = 0
    E[:, item] = 0
    E = E.tocsr()
    E.eliminate_zeros(); E.sort_indices()
    return X, D, users, item, E, n_gone


@pytest.mark.parametrize("case", ["pg-f32-k50", "cg-f64-k50", "tncg-f64-k50"])
def test_the_smaller_session_is_a_fresh_session(case):
    method, prec, k, maxupd, _ = CASES[case]
    X, D, gone_users, gone_item, E, n_gone = two_sided_removal(prec)
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    users = np.arange(0, dimA, 3)
    touched_u = np.union1d(np.unique(D.row), gone_users)
    touched_i = np.union1d(np.unique(D.col), gone_item)
    s, f = session_of(X, k, prec), session_of(E, k, prec)
    try:
        p, cd = params_for(s, case)
        for x in (s, f):
            assert x.set_segments(1, 4) == 4
        s.set_factors(A0, B0)
        s.topn_batch(users, 10, exclude_seen=True, output_score=True)   # (the row pointers exclude_seen keeps have been fetched once)
        assert s.subtract(D) == n_gone
        assert s.forget(1, gone_users) + s.forget(0, gone_item) == total(X, sp.coo_matrix(X.shape), prec).nnz - n_gone - E.nnz
        holds(s, E, "after the removals")
        assert (np.diff(E.indptr) == 0).sum() >= 3
        assert [s.segment_rows(1, j) for j in range(4)] == [f.segment_rows(1, j) for j in range(4)]
        out = []
        for x in (s, f):
            x.set_factors(A0, B0)
            top = x.topn_batch(users, 10, exclude_seen=True, output_score=True)
            llk0 = x.llk()
            x.half_sweep_rows(1, touched_u, p, 1e-7, cd)
            x.half_sweep_rows(0, touched_i, p, 1e-7, cd)
            Ar, Br = x.get_factors()
            x.set_factors(A0, B0)
            x.half_sweep(0, p, 1e-7, cd)
            B1 = x.get_factors()[1]
            x.half_sweep(1, p, 1e-7, cd)
            A, B = x.get_factors()
            out.append(dict(A=A, B=B, B1=B1, Ar=Ar, Br=Br, llk0=llk0, llk=x.llk(), top=top, plan=(x.plan(0), x.plan(1))))
        m, w = out
        assert np.array_equal(m["top"][0], w["top"][0])
        same_bits(m["top"][1], w["top"][1], "top-N scores")
        assert m["llk0"] == w["llk0"] and m["llk"] == w["llk"] and np.isfinite(m["llk"])
        same_bits(m["B1"], w["B1"], "B after the B half")
        same_bits(m["A"], w["A"], "A after the A half")
        same_bits(m["Ar"], w["Ar"], "A after the listed rows")
        same_bits(m["Br"], w["Br"], "B after the listed rows")
        assert not np.array_equal(m["Ar"][touched_u], A0[touched_u])
        assert m["plan"] == w["plan"]
        # exclude_seen has forgotten the cells: what the removals freed may be recommended again, what is still stored may not
        seen = E.toarray() > 0
        assert not seen[users[:, None], m["top"][0].astype(np.int64)].any()
    finally:
        s.close(); f.close()


# ---- 8. retract -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove", [False, True], ids=["subtract", "remove"])
@pytest.mark.parametrize("case", ["pg-f32-k50", "tncg-f64-k50"])
def test_retract_is_subtract_and_two_calls_over_listed_rows(case, remove):
    method, prec, k, maxupd, _ = CASES[case]
    X, D, _, _, _, n_gone = two_sided_removal(prec)
    dimA, dimB = X.shape
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    users, items = np.unique(D.row), np.unique(D.col)
    s, f = session_of(X, k, prec), session_of(X, k, prec)
    try:
        p, _ = params_for(s, case)
        s.set_factors(A0, B0); f.set_factors(A0, B0)
        got = s.retract(D, p, 1e-7, remove=remove)
        assert np.array_equal(got[0], users) and np.array_equal(got[1], items)
        assert (f.remove(D) if remove else f.subtract(D)) == (600 if remove else n_gone)
        step = f.real(1e-7)
        cd = f.cnst_div(p.l2_reg, step)
        f.half_sweep_rows(1, users, p, step, cd)
        f.half_sweep_rows(0, items, p, step, cd)
        (A, B), (Af, Bf) = s.get_factors(), f.get_factors()
        same_bits(A, Af, "A"); same_bits(B, Bf, "B")
        for w in (0, 1):
            for a, b in zip(s.matrix(w), f.matrix(w)):
                assert np.array_equal(a, b)
        untouched_users = np.setdiff1d(np.arange(dimA), users)
        same_bits(A[untouched_users], A0[untouched_users], "rows of A the call does not name")
        assert not np.array_equal(A[users], A0[users])
    finally:
        s.close(); f.close()
