"""New users and items join a resident session on the device (include/poismf_hip.h section 2d): Session.append, adopt_new, append_users and
append_items.  Every assertion is bit equality, and the reference is always a FRESH Session.from_coo on the grown matrix at the grown shape
with set_factors of the grown factors -- never the appended session itself.  Counts are integer-valued unless a test says otherwise.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness
from tests import helpers as H
from tests.test_gpu_invariance import CASES, params_for
from tests.test_gpu_session_update import bits, holds, same_bits, session_of, total, unchanged

pytestmark = pytest.mark.gpu

DIMA, DIMB, HOT_ITEM, LONG_USER = 500, 400, 7, 100
LENGTHS = [17, 0, 300, 16, 1, 15, 64, 65]   # both sides of the length-class cuts at 16 and 64; n_new = 1: 17, n_new = 3: 17, 0, 300
N_NEW = (1, 3, 130)
SOLVER_CASES = ["pg-f32-k50", "cg-f64-k50", "tncg-f64-k50"]


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def counts(rng, n, integer=True):
    return 1.0 + np.floor(rng.gamma(1.0, 1.0, n)) if integer else rng.uniform(0.1, 9.0, n)


def base_problem(integer=True, seed=11):
    """X (500 x 400), about 12 000 stored cells -- several UPD_CHUNK = 4096 chunks of the scatter: item HOT_ITEM stored by nearly every user
    (a long CSC row), user LONG_USER with about 300 cells, the other users with 5 .. 40"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(DIMA):
        n = 300 if r == LONG_USER else int(rng.integers(5, 41))
        c = rng.choice(np.setdiff1d(np.arange(DIMB), [HOT_ITEM]), size=n - 1, replace=False)
        if r % 50 != 49:
            c = np.concatenate([c, [HOT_ITEM]])
        rows.append(np.full(len(c), r)); cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    return sp.coo_matrix((counts(rng, len(row), integer), (row, col)), shape=(DIMA, DIMB))


def new_rows(n_new, width, seed, must=(), integer=True):
    """n_new rows over `width` columns with LENGTHS in turn (a row of length 0 is stored by nobody); the columns `must` are in every row of
    15 or more cells: new users then store the hot item, new items are stored by the long user"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n_new):
        n = LENGTHS[i % len(LENGTHS)]
        keep = [m for m in must if n >= 15]
        c = np.concatenate([rng.choice(np.setdiff1d(np.arange(width), keep), size=n - len(keep), replace=False), keep]).astype(np.int64)
        rows.append(np.full(len(c), i)); cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = rng.permutation(len(row))   # (unsorted triplets: append sorts them)
    return sp.coo_matrix((counts(rng, len(row), integer)[order], (row[order], col[order])), shape=(n_new, width))


def grown(X, Xn, which):
    """the grown matrix: new users are rows below X, new items columns to its right"""
    return (sp.vstack([X.tocsr(), Xn.tocsr()]) if which else sp.hstack([X.tocsr(), Xn.tocsr().T])).tocoo()


def as_held(X, prec):
    return total(X, sp.coo_matrix(X.shape), prec)


def factors_for(n, k, prec, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (n, k)).astype(H.dtype_of(prec))


def fresh_of(X, k, prec, A, B):
    f = session_of(X, k, prec)
    f.set_factors(np.ascontiguousarray(A), np.ascontiguousarray(B))
    return f


def is_session(s, X, A, B, what):
    """s holds the matrix X in both orientations and the factors A, B, and says so on the Python object"""
    assert (s.dimA, s.dimB) == X.shape == (A.shape[0], B.shape[0]) and s.shardA == (0, s.dimA) and s.shardB == (0, s.dimB), what
    holds(s, as_held(X, s.use_float), what)
    As, Bs = s.get_factors()
    same_bits(As, A, what + ": A"); same_bits(Bs, B, what + ": B")


def same_sessions(s, f, what):
    """both matrices, the counts and the factors of s are those of the fresh session f"""
    assert (s.dimA, s.dimB) == (f.dimA, f.dimB), what
    for w in (0, 1):
        assert s.nnz(w) == f.nnz(w), what
        for got, want in zip(s.matrix(w), f.matrix(w)):
            assert got.dtype == want.dtype and np.array_equal(bits(got) if got.dtype.kind == "f" else got, bits(want) if want.dtype.kind == "f" else want), what
    for got, want, name in zip(s.get_factors(), f.get_factors(), "AB"):
        same_bits(got, want, f"{what}: {name}")


# ---- 1. the grown matrices and factors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["coo", "host"])
@pytest.mark.parametrize("k", [8, 32, 50])
def test_append_gives_the_fresh_session_s_matrices_and_factors(prec, k, how):
    """k = 8 (both precisions) and k = 50 fp32 keep a line-padded copy of each factor, k = 32 fp32 and k = 50 fp64 do not"""
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    for n_new in N_NEW:
        for which in (1, 0):
            Xn = new_rows(n_new, DIMB if which else DIMA, 100 + n_new, must=[HOT_ITEM] if which else [LONG_USER])
            F = factors_for(n_new, k, prec, 3)
            G = grown(X, Xn, which)
            Ag, Bg = (np.vstack([A0, F]), B0) if which else (A0, np.vstack([B0, F]))
            s, f = session_of(X, k, prec, how), None
            try:
                s.set_factors(A0, B0)
                assert s.append(which, Xn, factors=F) == (DIMA if which else DIMB)
                what = f"append({which}) of {n_new} rows, k = {k}, {how}"
                is_session(s, G, Ag, Bg, what)
                f = fresh_of(G, k, prec, Ag, Bg)
                same_sessions(s, f, what)
            finally:
                s.close()
                if f is not None:
                    f.close()


def test_empty_rows_then_add_of_their_cells(prec):
    """add refused a row index at or above dimA before: it must accept the new rows' numbers now"""
    k = 8
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    for which in (1, 0):
        Xn = new_rows(130, DIMB if which else DIMA, 7, must=[HOT_ITEM] if which else [LONG_USER])
        G = grown(X, Xn, which)
        only_new = (G.tocsr() - grown(X, sp.coo_matrix(Xn.shape), which).tocsr()).tocoo()
        s = session_of(X, k, prec)
        try:
            s.set_factors(A0, B0)
            with pytest.raises(ValueError):
                s.add(only_new)
            assert s.append(which, n_new=130) == (DIMA if which else DIMB)
            Z = np.zeros((130, k), A0.dtype)
            is_session(s, grown(X, sp.coo_matrix(Xn.shape), which), *((np.vstack([A0, Z]), B0) if which else (A0, np.vstack([B0, Z]))), "empty rows")
            assert s.add(only_new) == Xn.tocsr().nnz
            holds(s, as_held(G, prec), f"empty rows of half {which}, then add")
        finally:
            s.close()


def test_two_appends_then_forget_then_add(prec):
    k = 50
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Xu, Fu = new_rows(130, DIMB, 5, must=[HOT_ITEM]), factors_for(130, k, prec, 3)
    G1 = grown(X, Xu, 1)
    Xi, Fi = new_rows(3, DIMA + 130, 6, must=[LONG_USER, DIMA + 2]), factors_for(3, k, prec, 4)   # (the new items know the new users)
    G2 = grown(G1, Xi, 0)
    Ag, Bg = np.vstack([A0, Fu]), np.vstack([B0, Fi])
    s = session_of(X, k, prec)
    try:
        s.set_factors(A0, B0)
        assert s.append(1, Xu, factors=Fu) == DIMA and s.append(0, Xi, factors=Fi) == DIMB
        is_session(s, G2, Ag, Bg, "users, then items")
        f = fresh_of(G2, k, prec, Ag, Bg)
        try:
            same_sessions(s, f, "users, then items")
        finally:
            f.close()
        gone = np.array([DIMA + 2, LONG_USER, DIMA + 129])
        G3 = G2.tocsr().tolil()
        G3[gone] = 0
        G3 = G3.tocsr(); G3.eliminate_zeros()
        assert s.forget(1, gone) == G2.tocsr().nnz - G3.nnz
        holds(s, as_held(G3, prec), "after forget")
        back = G2.tocsr()[gone[0]].tocoo()
        D = sp.coo_matrix((back.data, (np.full(back.nnz, gone[0]), back.col)), shape=G2.shape)
        assert s.add(D) == back.nnz
        holds(s, as_held((G3 + D.tocsr()).tocoo(), prec), "after forget and add")
        same_bits(s.get_factors()[0], Ag, "A")
    finally:
        s.close()


def test_non_integer_values(prec):
    k = 8
    X = base_problem(integer=False)
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    for which in (1, 0):
        Xn = new_rows(130, DIMB if which else DIMA, 9, must=[HOT_ITEM] if which else [LONG_USER], integer=False)
        F = factors_for(130, k, prec, 3)
        s = session_of(X, k, prec)
        try:
            s.set_factors(A0, B0)
            s.append(which, Xn, factors=F)
            is_session(s, grown(X, Xn, which), *((np.vstack([A0, F]), B0) if which else (A0, np.vstack([B0, F]))), f"non-integer values, half {which}")
        finally:
            s.close()


# ---- 2. the grown session behaves as a fresh one ------------------------------------------------------------------------------------------
def both_grown(case, prec, k, sweep_first=True, segments=3, profile=False):
    """s: a session on X with 3 segments of its A half, both halves swept once (so the padded copies are fresh and every scratch area has
    been used), then 130 users and 3 items appended; f: the fresh session on the grown matrix with the grown factors.  Returns (s, f, p,
    cd, Ag, Bg, new users, new items)."""
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Xu, Fu = new_rows(130, DIMB, 5, must=[HOT_ITEM]), factors_for(130, k, prec, 3)
    Xi, Fi = new_rows(3, DIMA + 130, 6, must=[LONG_USER, DIMA + 2]), factors_for(3, k, prec, 4)
    G = grown(grown(X, Xu, 1), Xi, 0)
    s = session_of(X, k, prec)
    p, cd = params_for(s, case)
    s.set_factors(A0, B0)
    if profile:
        s.profile(True)
    assert s.set_segments(1, segments) == segments
    if sweep_first:
        s.half_sweep(0, p, 1e-7, cd); s.half_sweep(1, p, 1e-7, cd)
        s.llk()
        s.topn_batch(np.arange(0, DIMA, 7), 10, exclude_seen=True)
    A1, B1 = s.get_factors()
    s.append(1, Xu, factors=Fu); s.append(0, Xi, factors=Fi)
    Ag, Bg = np.vstack([A1, Fu]), np.vstack([B1, Fi])
    f = fresh_of(G, k, prec, Ag, Bg)
    assert f.set_segments(1, segments) == segments
    return s, f, p, cd, Ag, Bg, np.arange(DIMA, DIMA + 130), np.arange(DIMB, DIMB + 3)


@pytest.mark.parametrize("sweep_first", [True, False], ids=["copies-fresh", "copies-stale"])
@pytest.mark.parametrize("case", SOLVER_CASES)
def test_the_grown_session_is_a_fresh_session(case, sweep_first):
    method, prec, k, maxupd, _ = CASES[case]
    s, f, p, cd, Ag, Bg, users, items = both_grown(case, prec, k, sweep_first)
    try:
        assert [s.segment_rows(1, j) for j in range(3)] == [f.segment_rows(1, j) for j in range(3)]
        assert s.segment_rows(1, 2)[1] == DIMA + 130
        same_sessions(s, f, case)
        # s goes on from what the append left on the device -- its padded copies included --, f from set_factors
        out = []
        for x in (s, f):
            x.half_sweep(0, p, 1e-7, cd)
            B1 = x.get_factors()[1]
            x.half_sweep(1, p, 1e-7, cd)
            A1 = x.get_factors()[0]
            out.append(dict(B1=B1, A1=A1, llk=x.llk(), plan=(x.plan(0), x.plan(1))))
        m, w = out
        same_bits(m["B1"], w["B1"], f"{case}: B after the B half")
        same_bits(m["A1"], w["A1"], f"{case}: A after the A half")
        assert m["plan"] == w["plan"]
        assert m["llk"] == w["llk"] and np.isfinite(m["llk"])
        assert np.isfinite(m["A1"]).all() and m["A1"][users].any() and m["B1"][items].any()
        # the new rows alone: those rows of the full half-sweep from the same start
        s.set_factors(Ag, Bg)
        s.half_sweep_rows(1, users, p, 1e-7, cd)
        A, B = s.get_factors()
        f.set_factors(Ag, Bg)
        f.half_sweep(1, p, 1e-7, cd)
        same_bits(A[users], f.get_factors()[0][users], f"{case}: the new users alone")
        same_bits(A[:DIMA], Ag[:DIMA], f"{case}: the old users"); same_bits(B, Bg, "B")
        s.set_factors(Ag, Bg)
        s.half_sweep_rows(0, items, p, 1e-7, cd)
        f.set_factors(Ag, Bg)
        f.half_sweep(0, p, 1e-7, cd)
        same_bits(s.get_factors()[1][items], f.get_factors()[1][items], f"{case}: the new items alone")
    finally:
        s.close(); f.close()


# ---- 3. serving -----------------------------------------------------------------------------------------------------------------------------
def test_serving_sees_the_new_rows(prec):
    case, k = "pg-f32-k50", 50
    s, f, p, cd, Ag, Bg, users, items = both_grown(case, prec, k)
    try:
        rng = np.random.default_rng(8)
        test = sp.csr_matrix((np.ones(260), (np.repeat(np.arange(130), 2), rng.integers(0, DIMB + 3, 260))), shape=(130, DIMB + 3))
        ix_u, ix_i = np.concatenate([users, [0, 5]]), np.concatenate([rng.integers(0, DIMB, 130), items[:2]])
        got, want = [], []
        for x, out in ((s, got), (f, want)):
            out.append(x.topn_batch(users, 10, exclude_seen=True, output_score=True))
            out.append(x.rank_batch(users, test, exclude_seen=True))
            out.append((x.predict(ix_u, ix_i),))
            out.append(x.similar_items(items, 5, output_score=True))
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
        assert (got[0][0].astype(np.int64) >= DIMB).any()   # a new item is recommended to a new user
    finally:
        s.close(); f.close()


# ---- 4. the guest follows B ---------------------------------------------------------------------------------------------------------------
def widened(rows, width):
    rows = rows.tocsr()
    return sp.csr_matrix((rows.data, rows.indices, rows.indptr), shape=(rows.shape[0], width))


@pytest.mark.parametrize("case", ["pg-f32-k50", "tncg-f64-k50"])
def test_the_guest_follows_a_grown_B(case):
    method, prec, k, maxupd, _ = CASES[case]
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Xi, Fi = new_rows(130, DIMA, 6, must=[LONG_USER]), factors_for(130, k, prec, 4)
    guests = new_rows(8, DIMB, 12, must=[HOT_ITEM]).tocsr()
    s, h = session_of(X, k, prec), session_of(X, k, prec)
    f = fresh_of(grown(X, Xi, 0), k, prec, A0, np.vstack([B0, Fi]))
    try:
        p, _ = params_for(s, case)
        call = lambda x, rows: x.topn_new(rows, p, 3, top_n=5, output_score=True, return_factors=True)
        s.set_factors(A0, B0); h.set_factors(A0, B0)
        first = call(s, guests)
        s.append(0, Xi, factors=Fi)
        second, want = call(s, widened(guests, DIMB + 130)), call(f, widened(guests, DIMB + 130))
        for a, b in zip(second, want):
            assert np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
        for a, b in zip(first, call(h, guests)):   # (and what the first call returned is what a session that never grew returns)
            assert np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
    finally:
        s.close(); h.close(); f.close()


# ---- 5. adopt_new -------------------------------------------------------------------------------------------------------------------------
def raw_adopt(s):
    first, n = C.c_size_t(0), C.c_size_t(0)
    return s.lib.poismf_hip_session_adopt_new(s.h, C.byref(first), C.byref(n))


def raw_fold_in(s, p, data, indptr, indices, Bsum, Amean):
    """poismf_hip_session_factors_new past the binding, which would sort the rows"""
    dt = H.dtype_of(s.use_float)
    data, Bsum, Amean = (np.ascontiguousarray(a, dtype=dt) for a in (data, Bsum, Amean))
    indptr, indices = np.ascontiguousarray(indptr, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint64)
    out = np.empty((len(indptr) - 1, s.k), dt)
    assert s.lib.poismf_hip_session_factors_new(s.h, api._ptr(data), api._ptr(indptr), api._ptr(indices), len(indptr) - 1, api._ptr(Bsum),
                                                api._ptr(Amean), C.byref(p), 3, api._ptr(out)) == 0
    return out


@pytest.mark.parametrize("case", SOLVER_CASES)
def test_adopt_new_is_append_of_the_fold_in_s_factors(case):
    method, prec, k, maxupd, _ = CASES[case]
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Bsum, Amean = B0.sum(axis=0), A0.mean(axis=0)
    rows = new_rows(130, DIMB, 5, must=[HOT_ITEM]).tocsr()
    s, t = session_of(X, k, prec), session_of(X, k, prec)
    try:
        p, cd = params_for(s, case)
        call = lambda x: x.topn_new(rows, p, 3, top_n=5, output_score=True, return_factors=True, Bsum=Bsum, Amean=Amean)
        s.set_factors(A0, B0); t.set_factors(A0, B0)
        before = call(s)
        assert s.adopt_new() == (DIMA, 130)
        assert t.append(1, rows, factors=before[2]) == DIMA
        same_sessions(s, t, f"{case}: adopt_new against append")
        is_session(s, grown(X, rows, 1), np.vstack([A0, before[2]]), B0, f"{case}: adopt_new")
        for a, b in zip(call(s), before):   # the guest is left as it was
            assert np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
        for x in (s, t):
            x.half_sweep(0, p, 1e-7, cd); x.half_sweep(1, p, 1e-7, cd)
        same_sessions(s, t, f"{case}: the sweep after adopt_new")
    finally:
        s.close(); t.close()


def test_adopt_new_refuses(prec):
    k = 8
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    s = session_of(X, k, prec)
    try:
        p, _ = params_for(s, "pg-f32-k50")
        s.set_factors(A0, B0)
        before = [s.matrix(w) for w in (0, 1)]
        assert raw_adopt(s) == 5                                             # no guest
        with pytest.raises(ValueError):
            s.adopt_new()
        Bsum, Amean = B0.sum(axis=0), A0.mean(axis=0)
        raw_fold_in(s, p, [1.0, 2.0, 3.0], [0, 2, 3], [9, 4, 1], Bsum, Amean)   # a descending guest row
        assert raw_adopt(s) == 5
        raw_fold_in(s, p, [1.0, 0.0, 3.0], [0, 2, 3], [4, 9, 1], Bsum, Amean)   # a stored zero
        assert raw_adopt(s) == 4
        unchanged(s, before)
        assert (s.dimA, s.dimB) == (DIMA, DIMB)
        same_bits(s.get_factors()[0], A0, "A")
        raw_fold_in(s, p, [1.0, 2.0, 3.0], [0, 2, 3], [4, 9, 1], Bsum, Amean)
        assert s.adopt_new() == (DIMA, 2)
    finally:
        s.close()


# ---- 6. the wrappers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pg-f32-k50", "tncg-f64-k50"])
def test_append_users_and_append_items_are_their_steps(case):
    method, prec, k, maxupd, _ = CASES[case]
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Bsum, Amean = B0.sum(axis=0), A0.mean(axis=0)
    Xu, Fu = new_rows(130, DIMB, 5, must=[HOT_ITEM]), factors_for(130, k, prec, 3)
    Xi = new_rows(3, DIMA + 260, 6, must=[LONG_USER, DIMA + 2])
    start = B0.mean(axis=0)
    s, t = session_of(X, k, prec), session_of(X, k, prec)
    try:
        p, _ = params_for(s, case)
        s.set_factors(A0, B0); t.set_factors(A0, B0)
        assert np.array_equal(s.append_users(Xu, p, 3, Bsum=Bsum, Amean=Amean), np.arange(DIMA, DIMA + 130))
        t.transform(Xu, p, 3, Bsum=Bsum, Amean=Amean)
        assert t.adopt_new() == (DIMA, 130)
        assert np.array_equal(s.append_users(Xu, p, 3, factors=Fu), np.arange(DIMA + 130, DIMA + 260))
        assert t.append(1, Xu, factors=Fu) == DIMA + 130
        same_sessions(s, t, "append_users")
        assert np.array_equal(s.append_items(Xi, p, 1e-7, start=start), np.arange(DIMB, DIMB + 3))
        assert t.append(0, Xi, factors=np.tile(start, (3, 1))) == DIMB
        step = t.real(1e-7)
        t.half_sweep_rows(0, np.arange(DIMB, DIMB + 3), p, step, t.cnst_div(p.l2_reg, step))
        same_sessions(s, t, "append_items")
        B = s.get_factors()[1]
        assert not np.array_equal(B[DIMB:], np.tile(start, (3, 1)))
        same_bits(B[:DIMB], B0, "the old items")
    finally:
        s.close(); t.close()


# ---- 7. refusals leave the session as it was --------------------------------------------------------------------------------------------
def raw_append(s, which, n_new, F, val, indptr, indices):
    dt = H.dtype_of(s.use_float)
    first = C.c_size_t(0)
    F = None if F is None else np.ascontiguousarray(F, dtype=dt)
    val = np.ascontiguousarray(val, dtype=dt)
    indptr, indices = np.ascontiguousarray(indptr, dtype=np.uint64), np.ascontiguousarray(indices, dtype=np.uint64)
    return s.lib.poismf_hip_session_append_rows(s.h, which, n_new, None if F is None else api._ptr(F), api._ptr(val), api._ptr(indptr),
                                                api._ptr(indices), C.byref(first))


def test_refusals_leave_the_session_as_it_was(prec):
    k = 8
    dimA, dimB = 57, 83
    rng = np.random.default_rng(1)
    X = sp.coo_matrix((counts(rng, 400), (rng.integers(0, dimA, 400), rng.integers(0, dimB, 400))), shape=(dimA, dimB))
    A0, B0 = factors_for(dimA, k, prec, 1), factors_for(dimB, k, prec, 2)
    guests = sp.csr_matrix(([1.0, 2.0, 1.0], ([0, 0, 1], [3, 80, 5])), shape=(2, dimB))
    good = dict(F=np.ones((2, k)), val=[1.0, 2.0, 3.0], indptr=[0, 2, 3], indices=[4, 9, 1])

    def refused(s, rc, which=1, **kw):
        assert raw_append(s, which, 2, **{**good, **kw}) == rc, kw

    s = session_of(X, k, prec)
    try:
        p, _ = params_for(s, "pg-f32-k50")
        s.set_factors(A0, B0)
        call = lambda: s.topn_new(guests, p, 3, top_n=5, output_score=True, return_factors=True, Bsum=B0.sum(axis=0), Amean=A0.mean(axis=0))
        guest = call()
        before = [s.matrix(w) for w in (0, 1)]
        refused(s, 3, indices=[4, dimB, 1])               # a minor index equal to the other dimension
        refused(s, 3, which=0, indices=[4, dimA, 1])
        refused(s, 3, indices=[9, 4, 1])                  # a descending row
        refused(s, 3, indices=[4, 4, 1])                  # ... and one that is not strictly ascending
        refused(s, 3, indptr=[0, 3, 2])                   # decreasing pointers
        for v in (0.0, -1.0, np.nan, np.inf):
            refused(s, 4, val=[1.0, v, 3.0])
        unchanged(s, before)
        assert s.nnz(0) == s.nnz(1) == len(before[0][0])
        assert len(s.matrix(1)[2]) == dimA + 1 and len(s.matrix(0)[2]) == dimB + 1
        for got, want, name in zip(s.get_factors(), (A0, B0), "AB"):
            same_bits(got, want, name)
        for a, b in zip(call(), guest):
            assert np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
        assert raw_append(s, 1, 2, **good) == 0           # (and the good rows are taken)
        assert s.nnz(1) == len(before[0][0]) + 3
    finally:
        s.close()

    csr, csc = harness.process_data(X.tocoo(), prec)
    s = api.Session(csr, csc, dimA, dimB, k, prec, shardA=(0, 30))     # a sharded session
    try:
        before = [s.matrix(w) for w in (0, 1)]
        refused(s, 5)
        with pytest.raises(ValueError):
            s.append(1, guests)
        unchanged(s, before)
        assert (s.dimA, s.shardA) == (dimA, (0, 30))
    finally:
        s.close()

    for side in (0, 1):                                            # one descending row in the host CSC / CSR
        cs = [[a.copy() for a in csc], [a.copy() for a in csr]]
        val, ind, ptr = cs[side]
        r = int(np.flatnonzero(np.diff(ptr.astype(np.int64)) >= 2)[0])
        p0 = int(ptr[r])
        ind[[p0, p0 + 1]] = ind[[p0 + 1, p0]]
        val[[p0, p0 + 1]] = val[[p0 + 1, p0]]
        s = api.Session(cs[1], cs[0], dimA, dimB, k, prec)
        try:
            before = [s.matrix(w) for w in (0, 1)]
            refused(s, 5)
            refused(s, 5, which=0, indices=[4, 9, 1])
            unchanged(s, before)
        finally:
            s.close()


# ---- 8. a profiling session ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cg-f64-k50", "cg-f32-k50"])   # (PG's rows record no decisions)
def test_a_profiling_session_keeps_its_counters_and_zeroes_the_new_rows(case):
    method, prec, k, maxupd, _ = CASES[case]
    X = base_problem()
    A0, B0 = factors_for(DIMA, k, prec, 1), factors_for(DIMB, k, prec, 2)
    Xu, Fu = new_rows(130, DIMB, 5, must=[HOT_ITEM]), factors_for(130, k, prec, 3)
    Xi, Fi = new_rows(3, DIMA + 130, 6, must=[LONG_USER, DIMA + 2]), factors_for(3, k, prec, 4)
    Ag, Bg = np.vstack([A0, Fu]), np.vstack([B0, Fi])
    s = session_of(X, k, prec)
    f = fresh_of(grown(grown(X, Xu, 1), Xi, 0), k, prec, Ag, Bg)
    try:
        p, cd = params_for(s, case)
        s.set_factors(A0, B0)
        s.profile(True); f.profile(True)
        s.half_sweep(0, p, 1e-7, cd); s.half_sweep(1, p, 1e-7, cd)
        old = [s.decisions(w) for w in (0, 1)]
        assert old[1][1].any() and old[0][1].any()
        s.append(1, Xu, factors=Fu); s.append(0, Xi, factors=Fi)
        for w, dim, n in ((1, DIMA, 130), (0, DIMB, 3)):
            now = s.decisions(w)
            for got, was in zip(now, old[w]):
                assert len(got) == dim + n and np.array_equal(got[:dim], was) and not got[dim:].any()
        for x in (s, f):
            x.set_factors(Ag, Bg)
            x.half_sweep(0, p, 1e-7, cd); x.half_sweep(1, p, 1e-7, cd)
        for w in (0, 1):
            for got, want in zip(s.decisions(w), f.decisions(w)):
                assert np.array_equal(got, want)
            assert s.decisions(w)[1][-3:].any()
        assert s.eval_stats(1) != (0, 0)
    finally:
        s.close(); f.close()
