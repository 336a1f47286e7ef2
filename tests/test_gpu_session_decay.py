"""Session.decay on the device (include/poismf_hip.h section 2e): every resident count scaled by gamma and per-user / per-item factors, what
fades to or below the floor leaving both orientations.  Every assertion is bit equality against tests/session_scale_values.py's expected(),
which holds no GPU code: ((x * gamma) * users[u]) * items[i] as three numpy multiplications in the model's dtype, kept iff > floor.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.session_scale_values import expected
from tests.test_gpu_invariance import CASES, params_for
from tests.test_gpu_session_remove import snapshot, unchanged
from tests.test_gpu_session_update import DIMA1, DIMB1, HOT, big_problem, holds, same_bits, session_of, small_counts, total, two_sided

pytestmark = pytest.mark.gpu
CHUNK = 4096   # UPD_CHUNK of poismf_amd/csrc/session_merge.hpp: consecutive resident entries one workgroup walks


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def decayed(X, prec, what, how="coo", k=4, **kw):
    """a session on X after decay(**kw): both orientations are expected()'s matrix and the call returns the cells that left"""
    E, n_gone, bad = expected(X, kw.get("gamma", 1.0), kw.get("users"), kw.get("items"), kw.get("floor", 0.0), prec)
    assert not bad
    s = session_of(X, k, prec, how)
    try:
        assert s.decay(**kw) == n_gone, what
        holds(s, E, what)
    finally:
        s.close()
    return E, n_gone


# ---- 1. nothing leaves: the values are rewritten in place ------------------------------------------------------------------------------
def test_nothing_leaves(prec):
    X, _ = big_problem()
    E, n_gone, bad = expected(X, 0.5, None, None, 0.0, prec)
    assert n_gone == 0 and not bad
    k = 8
    A0, B0 = harness.initialize_matrices(DIMA1, DIMB1, k, prec, 9)
    s = session_of(X, k, prec)
    try:
        p, cd = s.make_params("cg", 1e4, maxupd=5), s.cnst_div(1e4, 1e-7)
        s.set_factors(A0, B0)
        s.half_sweep(0, p, 1e-7, cd)
        s.half_sweep(1, p, 1e-7, cd)
        plans, nnz = (s.plan(0), s.plan(1)), (s.nnz(0), s.nnz(1))
        assert plans[0] and plans[1]
        assert s.decay(0.5) == 0
        holds(s, E, "decay(0.5)")
        assert (s.nnz(0), s.nnz(1)) == nnz and (s.plan(0), s.plan(1)) == plans
    finally:
        s.close()


# ---- 2. a floor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["coo", "host"])
def test_a_floor(prec, how):
    X, _ = big_problem()
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    E, n_gone, _ = expected(X, 0.5, None, None, 0.75, prec)
    assert n_gone == int((Xs.data == 1).sum()) and E.nnz == int((Xs.data >= 2).sum()) and n_gone > Xs.nnz // 4   # exactly the cells holding 1 leave
    assert ((np.diff(Xs.indptr) > 0) & (np.diff(E.indptr) == 0)).any()
    assert ((np.diff(Xs.tocsc().indptr) > 0) & (np.diff(E.tocsc().indptr) == 0)).any()
    decayed(X, prec, f"decay(0.5, floor=0.75) ({how})", how, k=8, gamma=0.5, floor=0.75)


# ---- 3. vectors, and the order of the roundings ----------------------------------------------------------------------------------------
def test_vectors_and_rounding_order(prec):
    X, _ = big_problem(integer=False)
    rng = np.random.default_rng(17)
    users, items = rng.uniform(0.3, 1.7, DIMA1), rng.uniform(0.3, 1.7, DIMB1)
    E, n_gone = decayed(X, prec, "vectors", k=8, gamma=0.9, floor=0.5, users=users, items=items)
    assert 0 < n_gone < X.nnz
    dt = H.dtype_of(prec)
    coo = total(X, sp.coo_matrix(X.shape), prec).tocoo()
    other = coo.data * (dt(0.9) * users.astype(dt)[coo.row] * items.astype(dt)[coo.col])   # (another association gives other bits somewhere)
    assert (other != ((coo.data * dt(0.9)) * users.astype(dt)[coo.row]) * items.astype(dt)[coo.col]).any()


# ---- 4. zeros in the vectors -----------------------------------------------------------------------------------------------------------
def test_zeros_in_the_vectors(prec):
    X, _ = big_problem()
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    rows = np.array([0, 101, 200, DIMA1 - 1])
    rng = np.random.default_rng(18)
    users, items = rng.uniform(0.5, 1.0, DIMA1), rng.uniform(0.5, 1.0, DIMB1)
    users[rows] = 0
    items[HOT] = 0
    E, _ = decayed(X, prec, "zeros in both vectors", k=8, gamma=1.0, floor=0.0, users=users, items=items)
    assert not np.diff(E.indptr)[rows].any() and E.tocsc()[:, HOT].nnz == 0 and E.nnz > 0
    only = np.ones(DIMA1)
    only[rows] = 0
    s, f = session_of(X, 8, prec), session_of(X, 8, prec)
    try:
        gone = s.decay(users=only)
        assert gone == f.forget(1, rows) == int(np.diff(Xs.indptr)[rows].sum())
        for w in (0, 1):
            for a, b in zip(s.matrix(w), f.matrix(w)):
                assert a.dtype == b.dtype and np.array_equal(a, b)
    finally:
        s.close(); f.close()


# ---- 5. edges of the chunking ----------------------------------------------------------------------------------------------------------
def filter_problem(keep, shape=None):
    """entries p = 0 .. len(keep) - 1 in CSR order, 64 to a row unless a shape is given (one row, or one cell per row); value 2 where keep"""
    n = len(keep)
    p = np.arange(n)
    if shape is None:
        shape, r, c = ((n + 63) // 64, 64), p // 64, p % 64
    elif shape[0] == 1:
        r, c = np.zeros(n, np.int64), p
    else:
        r, c = p * (shape[0] // n), np.zeros(n, np.int64)    # (shape[0] a multiple of n: empty rows in between)
    return sp.coo_matrix((np.where(keep, 2.0, 1.0), (r, c)), shape=shape)


def masks():
    rng = np.random.default_rng(19)
    m = {}
    for n in (4095, 4096, 4097, 8193):
        m[f"nnz {n}"] = rng.random(n) < 0.5
    first, last = np.zeros(8193, bool), np.zeros(8193, bool)
    first[0], last[-1] = True, True
    m["only the first entry kept"], m["only the last entry kept"] = first, last
    second = np.arange(2 * CHUNK + 5) >= CHUNK
    m["the first chunk gone"], m["the first chunk kept"] = second, ~second
    even = np.arange(8193) % 2 == 0
    m["alternating, even kept"], m["alternating, odd kept"] = even, ~even    # across entries 255 | 256 and 4095 | 4096 either way
    return m


MASKS = masks()


@pytest.mark.parametrize("what", sorted(MASKS))
def test_edges_of_the_chunking(prec, what):
    keep = MASKS[what]
    E, n_gone = decayed(filter_problem(keep), prec, what, gamma=1.0, floor=1.5)
    assert n_gone == int((~keep).sum()) and (E.data == 2).all()


@pytest.mark.parametrize("shape", [(1, 4097), (4097, 1), (2 * 4097, 1)], ids=["one row", "4097 rows of one cell", "an empty row between any two"])
def test_one_row_and_rows_of_one_cell(prec, shape):
    rng = np.random.default_rng(20)
    keep = rng.random(4097) < 0.5
    E, n_gone = decayed(filter_problem(keep, shape), prec, "a pure filter", gamma=1.0, floor=1.5)
    assert n_gone == int((~keep).sum())
    # the same choice made by a vector over the long dimension, every cell holding 2: each entry must find its own row's factor
    X = filter_problem(np.ones(4097, bool), shape)
    vec = np.ones(max(shape))
    vec[(np.arange(4097) * (max(shape) // 4097))[~keep]] = 0.5
    kw = dict(items=vec) if shape[0] == 1 else dict(users=vec)
    E2, n_gone2 = decayed(X, prec, "a filter by vector", gamma=1.0, floor=1.5, **kw)
    assert n_gone2 == n_gone and (E2 != E).nnz == 0
    E3, n_gone3 = decayed(X, prec, "a vector, nothing leaves", gamma=1.0, floor=0.0, **kw)       # in place
    assert n_gone3 == 0 and set(np.unique(E3.data)) == {1.0, 2.0}


def test_a_chunk_over_tens_of_thousands_of_empty_rows(prec):
    dimA, dimB = 30000, 50
    rng = np.random.default_rng(21)
    r = np.repeat([0, 15000, 29999], dimB)
    X = sp.coo_matrix((rng.uniform(0.5, 4.0, 3 * dimB), (r, np.tile(np.arange(dimB), 3))), shape=(dimA, dimB))
    users, items = rng.uniform(0.3, 1.7, dimA), rng.uniform(0.3, 1.7, dimB)
    E, n_gone = decayed(X, prec, "three users among 30 000", gamma=0.9, floor=1.0, users=users, items=items)
    assert 0 < n_gone < X.nnz
    E, n_gone = decayed(X, prec, "three users among 30 000, in place", gamma=0.9, users=users, items=items)
    assert n_gone == 0


# ---- 6. everything leaves --------------------------------------------------------------------------------------------------------------
def test_everything_leaves(prec):
    X, D = small_counts(57, 83, 400, 1), small_counts(57, 83, 120, 8)
    Xs = total(X, sp.coo_matrix(X.shape), prec)
    s = session_of(X, 4, prec)
    try:
        assert s.decay(0.0) == Xs.nnz
        assert s.nnz(0) == 0 and s.nnz(1) == 0
        holds(s, sp.csr_matrix(X.shape, dtype=H.dtype_of(prec)), "decay(0.0)")
        assert s.decay(0.5) == 0
        Ds = total(D, sp.coo_matrix(X.shape), prec)
        assert s.add(D) == Ds.nnz
        holds(s, Ds, "add on the emptied matrix")
    finally:
        s.close()


# ---- 7. small and large magnitudes -----------------------------------------------------------------------------------------------------
def test_small_and_large_magnitudes(prec):
    dt = H.dtype_of(prec)
    tiny, big = float(np.finfo(dt).tiny), float(np.finfo(dt).max)
    least = float(np.nextafter(dt(0), dt(1)))                      # the smallest subnormal
    rng = np.random.default_rng(22)
    where = rng.permutation(57 * 83)[:600]
    X = sp.coo_matrix((rng.choice([0.25, 1.0, 3.0], 600), (where // 83, where % 83)), shape=(57, 83))
    E, n_gone = decayed(X, prec, "subnormal results", gamma=tiny / 16)
    assert n_gone == 0 and (E.data > 0).all() and (E.data < tiny).all() and len(np.unique(E.data)) == 3
    E, n_gone = decayed(X, prec, "0.25 times the smallest subnormal is 0", gamma=least)
    assert n_gone == int((X.data == 0.25).sum()) > 0 and set(np.unique(E.data)) == {dt(least), dt(3 * least)}
    Xb = sp.coo_matrix((np.where(X.data == 3.0, big / 2, X.data), (X.row, X.col)), shape=X.shape)
    users = np.ones(57)
    users[Xb.row[Xb.data == big / 2][0]] = 4.0
    assert expected(Xb, 1.0, users, None, 0.0, prec)[2]
    s = session_of(Xb, 4, prec)
    try:
        before = snapshot(s)
        with pytest.raises(ValueError, match="not finite"):
            s.decay(users=users)
        unchanged(s, before)
        users[users == 4.0] = 2.0
        assert s.decay(users=users) == 0                           # big / 2 * 2 is finite
        holds(s, expected(Xb, 1.0, users, None, 0.0, prec)[0], "just below the overflow")
    finally:
        s.close()


# ---- 8. a fresh session's bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [True, False], ids=["compacted", "in place"])
@pytest.mark.parametrize("case", ["pg-f32-k50", "cg-f64-k50", "tncg-f64-k50"])
def test_the_decayed_session_is_a_fresh_session(case, leaves):
    method, prec, k, maxupd, _ = CASES[case]
    X, _ = two_sided()
    dimA, dimB = X.shape
    rng = np.random.default_rng(23)
    kw = dict(gamma=0.5, floor=0.75, users=rng.uniform(0.6, 1.4, dimA), items=rng.uniform(0.6, 1.4, dimB)) if leaves else \
        dict(gamma=0.9, users=rng.uniform(0.5, 1.0, dimA), items=rng.uniform(0.5, 1.0, dimB))
    E, n_gone, bad = expected(X, kw["gamma"], kw["users"], kw["items"], kw.get("floor", 0.0), prec)
    assert not bad and (n_gone > 500 if leaves else n_gone == 0)
    A0, B0 = harness.initialize_matrices(dimA, dimB, k, prec, 9)
    users = np.arange(0, dimA, 3)
    new_rows = small_counts(12, dimB, 150, 21).tocsr()
    s, f = session_of(X, k, prec), session_of(E, k, prec)
    try:
        p, cd = params_for(s, case)
        for x in (s, f):
            assert x.set_segments(1, 4) == 4
        s.set_factors(A0, B0)
        s.topn_batch(users, 10, exclude_seen=True, output_score=True)   # (the row pointers exclude_seen keeps have been fetched once)
        assert s.decay(**kw) == n_gone
        holds(s, E, "after the decay")
        assert [s.segment_rows(1, j) for j in range(4)] == [f.segment_rows(1, j) for j in range(4)]
        out = []
        for x in (s, f):
            x.set_factors(A0, B0)
            top = x.topn_batch(users, 10, exclude_seen=True, output_score=True)
            llk0 = x.llk()
            new = x.transform(new_rows, p, 3)
            x.half_sweep(0, p, 1e-7, cd)
            B1 = x.get_factors()[1]
            x.half_sweep(1, p, 1e-7, cd)
            A, B = x.get_factors()
            out.append(dict(A=A, B1=B1, llk0=llk0, llk=x.llk(), top=top, new=new, plan=(x.plan(0), x.plan(1))))
        m, w = out
        assert np.array_equal(m["top"][0], w["top"][0])
        same_bits(m["top"][1], w["top"][1], "top-N scores")
        assert m["llk0"] == w["llk0"] and m["llk"] == w["llk"] and np.isfinite(m["llk"])
        same_bits(m["new"], w["new"], "factors of new rows")
        same_bits(m["B1"], w["B1"], "B after the B half")
        same_bits(m["A"], w["A"], "A after the A half")
        assert m["plan"] == w["plan"]
        seen = E.toarray() > 0
        assert not seen[users[:, None], m["top"][0].astype(np.int64)].any()
    finally:
        s.close(); f.close()


# ---- 9. with the other updates ---------------------------------------------------------------------------------------------------------
def test_with_the_other_updates(prec):
    X, D = big_problem()
    E, n_gone, _ = expected(X, 0.5, None, None, 0.75, prec)
    created = total(E, D, prec).nnz - E.nnz
    s = session_of(X, 8, prec)
    try:
        assert s.decay(0.5, floor=0.75) == n_gone
        assert s.add(D) == created                                  # (halves of integers and integers: every sum is exact)
        holds(s, total(E, D, prec), "decay, then add(D)")
        assert s.subtract(D) == created
        holds(s, E, "decay, add(D), subtract(D)")
    finally:
        s.close()


def test_decay_after_append_users(prec):
    dt = H.dtype_of(prec)
    X = small_counts(57, 83, 400, 1)
    new_rows = small_counts(5, 83, 40, 3).tocsr()
    grown = sp.vstack([total(X, sp.coo_matrix(X.shape), prec), new_rows.astype(dt)]).tocsr()
    rng = np.random.default_rng(24)
    vec = rng.uniform(0.2, 1.2, 62)
    E, n_gone, _ = expected(grown, 0.8, vec, None, 0.9, prec)
    s = session_of(X, 4, prec)
    try:
        assert np.array_equal(s.append_users(new_rows, None, 0, factors=np.full((5, 4), 0.3, dt)), np.arange(57, 62))
        before = snapshot(s)
        with pytest.raises(ValueError):
            s.decay(0.8, floor=0.9, users=vec[:57])                  # the old length
        unchanged(s, before)
        assert s.decay(0.8, floor=0.9, users=vec) == n_gone and 0 < n_gone < grown.nnz
        holds(s, E, "append_users, then decay")
    finally:
        s.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def raw_scale(s, gamma, users, items, floor, count=True):
    dt = np.float32 if s.use_float else np.float64
    vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=dt)
    users, items = vec(users), vec(items)
    gone = C.c_size_t(99)
    rc = s.lib.poismf_hip_session_scale(s.h, gamma, None if users is None else api._ptr(users), None if items is None else api._ptr(items), floor,
                                        C.byref(gone) if count else None)
    return rc, gone.value


def test_refusals_leave_the_session_as_it_was(prec):
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 400, 1)
    csr, csc = harness.process_data(X.tocoo(), prec)
    for shard in (dict(shardA=(0, 30)), dict(shardB=(10, dimB))):    # a session that holds a shard
        s = api.Session(csr, csc, dimA, dimB, 4, prec, **shard)
        try:
            before = snapshot(s)
            with pytest.raises(ValueError, match="cannot be changed in place"):
                s.decay(0.5)
            assert raw_scale(s, 0.5, None, None, 0.0) == (5, 0)
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
            with pytest.raises(ValueError, match="cannot be changed in place"):
                s.decay(0.5, floor=0.75)
            assert raw_scale(s, 0.5, None, None, 0.75) == (5, 0)
            unchanged(s, before)
        finally:
            s.close()


def test_defaults_and_the_entry_point_itself(prec):
    dimA, dimB = 57, 83
    X = small_counts(dimA, dimB, 400, 1)
    s = session_of(X, 4, prec)
    try:
        before = snapshot(s)
        assert s.decay() == 0
        assert raw_scale(s, 1.0, None, None, 0.0) == (0, 0)
        bad = np.ones(dimA)
        for v in (-1.0, np.nan, np.inf):                               # past the binding's own checks
            assert raw_scale(s, v, None, None, 0.0)[0] == 4 and raw_scale(s, 0.5, None, None, v)[0] == 4
            bad[7] = v
            assert raw_scale(s, 0.5, bad, None, 0.0)[0] == 4 and raw_scale(s, 0.5, None, np.resize(bad, dimB), 0.0)[0] == 4
        big = np.ones(dimA)
        big[:] = np.finfo(H.dtype_of(prec)).max
        assert raw_scale(s, 2.0, big, None, 0.0) == (7, 0)
        unchanged(s, before)
        E, n_gone, _ = expected(X, 0.5, None, None, 0.75, prec)
        assert raw_scale(s, 0.5, None, None, 0.75, count=False)[0] == 0 and n_gone > 0     # n_removed = NULL
        holds(s, E, "the entry point with n_removed = NULL")
        assert raw_scale(s, 0.5, None, None, 0.0) == (0, 0)
        holds(s, expected(E, 0.5, None, None, 0.0, prec)[0], "and once more, counted")
    finally:
        s.close()
