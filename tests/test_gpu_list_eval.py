"""List-wise evaluation (include/poismf_hip.h section 1q) on the GPU: positions, fixed-point cosine sums, lengths and exposure against
the definition rebuilt from the library's independent path, over k, both precisions and six list widths; independence of the batch
and of the chunks; the session against the host-pointer entry; eval_lists on the plain top-N against eval_ranking's exact ranks; the
return codes.

The expectation (lists_expect; tests/test_list_eval_cpu.py defines it and holds it to hand-written answers): the chains from
predict_multiple(B, B, ., .) -- the pair_dot_kernel path, which the new kernel does not share --, the two multiplications as single
numpy operations in the model's precision, np.rint for the quantisation and integer sums.  Every device output is an integer: there is
no tolerance anywhere in this file."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, metrics
from tests import helpers as H
from tests.test_list_eval_cpu import lists_expect

pytestmark = pytest.mark.gpu

DIMA, DIMB, BATCH = 90, 700, 150      # 150 rows: 37 workgroups of four waves and a half-filled one
KS = (1, 7, 50, 130)                  # 130: a second 256-byte chunk of the gather in fp32 (the fifth in fp64)
WIDTHS = (1, 2, 10, 64, 65, 128)      # 1: no pair; 64 / 65: one owned position per lane against two, one gather pass against two
ZERO_ROWS = (213, 690)
NONE = api.TOPN_NONE
FORCED = {3: 0, 17: 1, 40: 2, 69: 63, 101: 64}   # row -> its length (cut to the width); every other row is full
LONG_ROW = 7                          # its held-out row has 300 cells: longer than a list and than a wave's stride


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


# ---- inputs (the shape of tests/test_gpu_topn_diverse.py's) ----
def make_factors(k, prec, seed=0, dimB=DIMB):
    """A [DIMA x k] and B [dimB x k]: rows 350 .. 449 of B repeat rows 0 .. 99 exactly (cosine 1), rows 450 .. 649 are rows 0 .. 199
    with each entry moved by about one percent (near-duplicates), ZERO_ROWS are zero (inverse norm 0: cosine 0).  k = 1: about 60 rows
    are positive, the others negative, so the cosines are +1 and -1."""
    rng = np.random.default_rng(1000 * k + seed)
    dt = H.dtype_of(prec)
    A = rng.random((DIMA, k)) ** 2 + 0.01
    if k == 1:
        B = -(0.001 + rng.random((dimB, 1)))
        pos = rng.choice(dimB, 60, replace=False)
        B[pos[:4], 0] = 0.8 + 0.2 * rng.random(4)
        B[pos[4:], 0] = 0.05 + 0.25 * rng.random(56)
    else:
        B = 2.0 * rng.random((dimB, k)) ** 4 + 2.0 ** -10
    B[350:450] = B[0:100]
    B[450:650] = B[0:200] * (1.0 + 0.01 * rng.standard_normal((200, k)))
    B[list(ZERO_ROWS)] = 0
    return np.ascontiguousarray(A, dtype=dt), np.ascontiguousarray(B, dtype=dt)


def batch_users(seed=0):
    """150 batch entries over 90 users: unordered, with repeats"""
    return np.random.default_rng(seed).integers(0, DIMA, BATCH).astype(np.uint64)


def chain_block(B, P):
    """predict_multiple(B, B, ., .) for every pair of the items P: [c x c]"""
    P = np.asarray(P, np.uint64)
    out = np.empty(len(P) * len(P), B.dtype)
    if len(P):
        api._predict_multiple(out, B, B, np.repeat(P, len(P)), np.tile(P, len(P)))
    return out.reshape(len(P), len(P))


def norms(B):
    """(the squared norms predict_multiple gives, their inverse roots as section 1p wants them)"""
    every = np.arange(B.shape[0], dtype=np.uint64)
    n2 = np.empty(B.shape[0], B.dtype)
    api._predict_multiple(n2, B, B, every, every)
    inv = np.zeros(B.shape[0], B.dtype)
    nz = n2 != 0
    inv[nz] = B.dtype.type(1) / np.sqrt(n2[nz])
    assert inv.dtype == B.dtype
    return n2, inv


def model_of(A, B, prec):
    m = api.PoisMF(k=A.shape[1], use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, A.shape[0], B.shape[0], True
    return m


def session_of(A, B, prec):
    dimA, dimB = A.shape[0], B.shape[0]
    row = np.arange(dimA)
    s = api.Session.from_coo(sp.coo_matrix((np.ones(dimA), (row, row % dimB)), shape=(dimA, dimB)), A.shape[1], prec)
    s.set_factors(A, B)
    return s


_SETUP = {}


def setup_of(k, prec):
    """(A, B, the chains among all items, squared norms, inverse norms), computed once per (k, precision) and left unchanged"""
    if (k, prec) not in _SETUP:
        A, B = make_factors(k, prec)
        n2, inv = norms(B)
        G = chain_block(B, np.arange(DIMB))
        for a in (A, B, G, inv, n2):
            a.setflags(write=False)
        _SETUP[k, prec] = A, B, G, n2, inv
    return _SETUP[k, prec]


def random_lists(width, seed=0):
    """150 rows of `width` distinct random items; the rows FORCED are cut to 0, 1, 2, 63 and 64 items and padded.  Rows 0 and 1 open with
    an item and its exact copy, and with the two zero rows."""
    rng = np.random.default_rng(100 * width + seed)
    lists = np.stack([rng.permutation(DIMB)[:width] for _ in range(BATCH)]).astype(np.uint64)
    if width >= 2:
        lists[0, :2] = (5, 355)
        lists[1, :2] = ZERO_ROWS
        for r in (0, 1):                                       # (keep the rows distinct)
            rest = np.setdiff1d(rng.permutation(DIMB), lists[r, :2], assume_unique=True)
            lists[r, 2:] = rest[:width - 2]
    for row, length in FORCED.items():
        lists[row, min(length, width):] = NONE
    return lists


def held_out(lists, seed=0):
    """A held-out row per list: empty for every fifth row; otherwise random items together with the list's first and last real entry;
    LONG_ROW has 300 cells; row 1 holds an item that only row 2 lists.  (indptr, indices) as uint64, rows strictly ascending."""
    rng = np.random.default_rng(seed + 7)
    rows = []
    for u, row in enumerate(lists):
        real = row[row != NONE].astype(np.int64)
        if u % 5 == 0:
            rows.append(np.empty(0, np.int64))
            continue
        cells = rng.choice(DIMB, 300 if u == LONG_ROW else int(rng.integers(1, 12)), replace=False)
        if len(real):
            cells = np.concatenate((cells, real[:1], real[-1:]))
        if u == 1:
            only_there = np.setdiff1d(lists[2][lists[2] != NONE].astype(np.int64), real)
            cells = np.concatenate((cells, only_there[:1]))
        rows.append(np.unique(cells))
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.uint64)


def same(got, want, what):
    assert len(got) == 4
    for name, g, w in zip(("pos", "cos_sum", "length", "exposure"), got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        assert g is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError((what, name, bad[:8].tolist(), g[bad[:4]].tolist(), w[bad[:4]].tolist()))


# ---- 1. the definition ----
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("k", KS)
def test_outputs_against_the_definition(prec, k, width):
    A, B, G, n2, inv = setup_of(k, prec)
    assert np.array_equal(B[350:450], B[0:100]) and not B[list(ZERO_ROWS)].any() and inv[ZERO_ROWS[0]] == 0
    chains = lambda P: G[np.ix_(P, P)]
    lists = random_lists(width)
    test = held_out(lists)
    want = lists_expect(lists, chains, inv, test, DIMB)
    got = api.list_eval(B, lists, test, item_norm=n2)
    same(got, want, f"k {k} width {width}")
    # the inputs do reach what they are meant to reach
    assert want[2].min() == 0 and want[2].max() == width and int(np.diff(test[0].astype(np.int64)).max()) >= 300
    real_len = want[2][np.repeat(np.arange(BATCH), np.diff(test[0].astype(np.int64)))]
    assert (want[0] == 0).any() and (want[0] == api.LIST_ABSENT).any() and (want[0] == real_len - 1).any()
    if width >= 2:
        one = 2 ** 40
        assert abs(int(want[1][0]) - one) <= (one >> 10) or width > 2          # row 0 at width 2: an item and its exact copy
        assert want[1][1] == 0 or width > 2                                      # row 1 at width 2: the two zero rows
        assert k == 1 or len(np.unique(want[1])) > BATCH // 2
    else:
        assert not want[1].any()
    if k == 1 and width >= 10:
        c = want[2].astype(np.int64)
        assert (want[1] < (c * (c - 1) // 2 - 1) * 2 ** 40).any()                # rows of both signs: cosines of -1


@pytest.mark.parametrize("width", (10, 128))
@pytest.mark.parametrize("k", KS)
def test_the_library_s_own_lists(prec, k, width):
    """what topN_batch and topN_diverse return, passed on as it is: near-duplicates next to each other, and the padded rows of
    topN_diverse where the exclusions leave fewer than `width` items"""
    A, B, G, n2, inv = setup_of(k, prec)
    users = batch_users()
    model = model_of(A, B, prec)
    chains = lambda P: G[np.ix_(P, P)]
    everything = np.arange(DIMB)
    excl = [np.empty(0, np.int64)] * BATCH
    excl[4], excl[9] = everything[:-3], everything                               # rows left with 3 items and with none
    indptr = np.zeros(BATCH + 1, np.uint64)
    indptr[1:] = np.cumsum([len(e) for e in excl])
    plain = model.topN_batch(users, width)[0]
    diverse = model.topN_diverse(users, width, min(2 * width, 200), 0.7, exclude=(indptr, np.concatenate(excl).astype(np.uint64)), item_norm=n2)[0]
    assert (diverse[9] == NONE).all() and (diverse[4] != NONE).sum() == 3
    for name, lists in (("topN_batch", plain), ("topN_diverse", diverse)):
        test = held_out(lists, seed=1)
        same(api.list_eval(B, lists, test, item_norm=n2), lists_expect(lists, chains, inv, test, DIMB), f"{name} k {k} width {width}")


# ---- 2. independence ----
def test_a_row_does_not_depend_on_the_batch(prec):
    A, B, G, n2, inv = setup_of(50, prec)
    lists = random_lists(65)
    test = held_out(lists)
    tp = test[0].astype(np.int64)
    s = session_of(A, B, prec)
    try:
        whole = s.list_eval(lists, test, item_norm=n2)
        same(whole, lists_expect(lists, lambda P: G[np.ix_(P, P)], inv, test, DIMB), "the batch of 150")
        total = np.zeros(DIMB, np.uint32)
        for u in range(BATCH):
            if u not in (0, 1, 2, LONG_ROW, 40, 69, 101, 148, 149) and u not in FORCED:
                total += np.bincount(lists[u][lists[u] != NONE].astype(np.int64), minlength=DIMB).astype(np.uint32)
                continue
            one_test = (np.array([0, tp[u + 1] - tp[u]], np.uint64), test[1][tp[u]:tp[u + 1]])
            pos, cos, length, expo = s.list_eval(lists[u:u + 1], one_test, item_norm=n2)
            assert np.array_equal(pos, whole[0][tp[u]:tp[u + 1]]) and cos[0] == whole[1][u] and length[0] == whole[2][u], u
            total += expo
        assert np.array_equal(total, whole[3])
        # a row twice: twice the exposure, the same answers
        twice = s.list_eval(np.concatenate((lists, lists[:1])), None, item_norm=n2)
        assert twice[1][-1] == whole[1][0] and np.array_equal(twice[3] - whole[3], np.bincount(lists[0].astype(np.int64), minlength=DIMB))
    finally:
        s.close()


@pytest.mark.parametrize("width", (10, 128))
def test_chunks_do_not_change_anything(prec, width):
    """a budget that leaves room for at most 40 rows per chunk: at least four chunks for the 150 rows"""
    A, B, G, n2, inv = setup_of(7, prec)
    lists = random_lists(width)
    test = held_out(lists)
    cells, real = len(test[1]), np.dtype(H.dtype_of(prec)).itemsize
    up = lambda v: (v + 31) // 32 * 32
    fixed = up(DIMB * real) + up(DIMB * 4)
    budget = fixed + 256 + 4 + 8 * cells + 40 * (4 * width + 16)
    lib = api.load_library(prec)
    bytes_for = lambda m, b: lib.poismf_hip_list_eval_scratch_bytes(m, width, cells, DIMB, b)
    size = bytes_for(BATCH, budget)
    print(f"width {width}: budget {budget} B, scratch {size} B, one chunk {bytes_for(BATCH, 0)} B")
    assert 0 < size <= budget
    # the scratch grows with the users until a chunk is full: it is full at 40 users, so the 150 rows take four chunks
    assert bytes_for(39, budget) < bytes_for(40, budget) == bytes_for(BATCH // 3, budget) == size
    assert bytes_for(BATCH - 1, 0) < bytes_for(BATCH, 0)                 # (while the default budget holds all the rows in one)
    assert api._list_eval_scratch(BATCH, width, cells, DIMB, budget, real)[:2] == (size, 40)
    one = api.list_eval(B, lists, test, item_norm=n2)
    same(api.list_eval(B, lists, test, item_norm=n2, budget_mb=(budget + 0.5) / 2 ** 20), one, f"chunks, width {width}")
    s = session_of(A, B, prec)
    try:
        same(s.list_eval(lists, test, item_norm=n2, budget_mb=(budget + 0.5) / 2 ** 20), one, f"chunks, session, width {width}")
        # room for one user only: 150 chunks
        least = fixed + 256 + 4 + 8 * cells + (4 * width + 16)
        assert lib.poismf_hip_list_eval_scratch_bytes(BATCH, width, cells, DIMB, least) > 0
        assert lib.poismf_hip_list_eval_scratch_bytes(BATCH, width, cells, DIMB, least - 1) == 0
        same(s.list_eval(lists, test, item_norm=n2, budget_mb=(least + 0.5) / 2 ** 20), one, f"one user per chunk, width {width}")
        with pytest.raises(ValueError, match="budget_mb"):
            s.list_eval(lists, test, item_norm=n2, budget_mb=(least - 0.5) / 2 ** 20)
    finally:
        s.close()


# ---- 3. the session, and the optional inputs ----
@pytest.mark.parametrize("k", (7, 130))
def test_session_equals_the_host_pointer_call(prec, k):
    A, B, G, n2, inv = setup_of(k, prec)
    s = session_of(A, B, prec)
    try:
        assert np.array_equal(s.item_norms(), n2)
        for width in (10, 128):
            lists = random_lists(width)
            test = held_out(lists)
            full = api.list_eval(B, lists, test, item_norm=n2)
            same(s.list_eval(lists, test, item_norm=n2), full, f"session, width {width}")
            for entry in (lambda *a, **kw: api.list_eval(B, *a, **kw), s.list_eval):
                same(entry(lists, None, item_norm=n2), (None,) + full[1:], "test=None")
                same(entry(lists, test), (full[0], None) + full[2:], "item_norm=None")
                same(entry(lists), (None, None) + full[2:], "neither")
        before = s.topn_batch(np.arange(DIMA), 10, output_score=True)
        s.list_eval(random_lists(64), item_norm=n2)
        after = s.topn_batch(np.arange(DIMA), 10, output_score=True)      # (the calls share the session's scratch)
        assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()
        A2, B2 = s.get_factors()
        assert A2.tobytes() == A.tobytes() and B2.tobytes() == B.tobytes()
    finally:
        s.close()


def test_r_flavour():
    """(the R flavour is double only)"""
    A, B, G, n2, inv = setup_of(50, False)
    lists = random_lists(10)
    test = held_out(lists)
    want = api.list_eval(B, lists, test, item_norm=n2)
    lib = api.load_library("r")
    as_int = lambda a: np.ascontiguousarray(np.where(a == NONE, np.uint64(2 ** 64 - 1), a).astype(np.int64).astype(np.int32))
    l32, tp, ti = as_int(lists), as_int(test[0]), as_int(test[1])
    assert (l32 == -1).sum() == (lists == NONE).sum()
    pos, cos = np.zeros(len(ti), np.uint32), np.zeros(BATCH, np.int64)
    length, expo = np.zeros(BATCH, np.uint32), np.ones(DIMB, np.uint32)
    p = api._ptr
    assert lib.poismf_hip_list_eval(p(B), 50, DIMB, p(l32), BATCH, 10, p(inv), p(tp), p(ti), 0, p(pos), p(cos), p(length), p(expo)) == 0
    same((pos, cos, length, expo), want, "R flavour")


# ---- 4. eval_lists on the plain top-N against the exact ranks ----
def test_eval_lists_of_the_plain_top_n_is_eval_ranking(prec):
    k, n = 7, 10
    A, B, G, n2, inv = setup_of(k, prec)
    rng = np.random.default_rng(11)
    model = model_of(A, B, prec)
    users = batch_users(seed=3)
    X = sp.random(DIMA, DIMB, density=0.05, random_state=1, format="csr")
    best = model.topN_batch(np.arange(DIMA), 40)[0].astype(np.int64)
    rows, cols = [], []
    for u in range(DIMA):
        if u % 6 == 0:
            continue                                                              # users without a held-out cell
        pick = np.concatenate((best[u, rng.choice(40, 6, replace=False)], rng.choice(DIMB, 4), X[u].indices[:2]))   # (some in X: excluded)
        rows += [u] * len(pick)
        cols += pick.tolist()
    X_test = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(DIMA, DIMB))
    X_test.sum_duplicates()
    assert X_test.multiply(X).nnz > 20 and (np.diff(X_test.indptr)[users.astype(np.int64)] == 0).any()
    items = model.topN_batch(users, n, exclude=X[users.astype(np.int64)])[0]
    want = model.eval_ranking(X_test, k=n, exclude=X, users=users, per_user=True)
    pop = np.asarray(X.getnnz(axis=0)).reshape(-1)
    s = session_of(A, B, prec)
    try:
        for who in (model, s):
            got = who.eval_lists(items, users, X_test, exclude=X, item_pop=pop, per_user=True)
            for name in metrics.LIST_METRICS:
                assert got["per_user"][name].dtype == np.float64
                assert np.array_equal(got["per_user"][name], want["per_user"][name], equal_nan=True), name
                assert got[name] == want[name], name
            assert got["n_users"] == want["n_users"] and 0 < got["n_users"] < BATCH and got["n_lists"] == BATCH
            assert 0 < got["hit"] < 1 and 0 < got["ild"] < 1 and 0 < got["coverage"] < 1 and 0 < got["gini"] < 1 and got["novelty"] > 0
            assert np.array_equal(got["length"], np.full(BATCH, n)) and got["exposure"].sum() == n * BATCH
            # the positions are the ranks wherever the rank is inside the list
            valid = want["ranks"] != api.RANK_EXCLUDED
            assert len(got["positions"]) == valid.sum()
            assert np.array_equal(got["positions"], np.where(want["ranks"][valid] < n, want["ranks"][valid], api.LIST_ABSENT))
        # a smaller k evaluates the lists' first columns; item_norm= given changes nothing
        five = model.eval_lists(items, users, X_test, k=5, exclude=X, item_norm=n2)
        want5 = model.eval_ranking(X_test, k=5, exclude=X, users=users)
        assert all(five[name] == want5[name] for name in metrics.LIST_METRICS)
        assert five == s.eval_lists(items[:, :5], users, X_test, exclude=X, item_norm=s.item_norms())
        # no held-out matrix: the list metrics are left out
        bare = s.eval_lists(items)
        assert set(bare) == {"ild", "coverage", "gini", "n_users", "n_lists"} and bare["ild"] == got["ild"] and bare["gini"] == got["gini"]
    finally:
        s.close()


# ---- 5. return codes ----
def test_return_code_2_leaves_the_outputs_untouched(prec):
    k = 7
    A, B, G, n2, inv = setup_of(k, prec)
    dt = H.dtype_of(prec)
    s = session_of(A, B, prec)
    lib = api.load_library(prec)
    p = api._ptr
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    ok = dict(lists=u64([[3, 1, 2], [5, 4, NONE]]), n=3, inv=inv, test=(u64([0, 2, 3]), u64([1, 4, 5])), budget=0, dimB=DIMB, k=k)
    bad_inv = lambda j, x: np.concatenate([inv[:j], np.array([x], dt), inv[j + 1:]])
    cases = {
        "repeated-entry": dict(lists=u64([[3, 1, 3], [5, 4, NONE]])), "entry-after-padding": dict(lists=u64([[3, 1, 2], [5, NONE, 4]])),
        "index-out-of-range": dict(lists=u64([[3, 1, DIMB], [5, 4, NONE]])), "width-0": dict(n=0), "width-129": dict(n=129),
        "inv-nan": dict(inv=bad_inv(3, np.nan)), "inv-inf": dict(inv=bad_inv(0, np.inf)), "inv-negative": dict(inv=bad_inv(DIMB - 1, -1e-30)),
        "test-descending": dict(test=(u64([0, 2, 3]), u64([4, 1, 5]))), "test-repeated": dict(test=(u64([0, 2, 3]), u64([4, 4, 5]))),
        "test-out-of-range": dict(test=(u64([0, 2, 3]), u64([4, DIMB, 5]))), "test-indptr-decreasing": dict(test=(u64([2, 3, 1]), u64([1, 4, 5]))),
        "budget-too-small": dict(budget=DIMB * (np.dtype(dt).itemsize + 4)), "too-many-items": dict(dimB=2 ** 24 + 1),
        "k-zero": dict(k=0), "k-too-large": dict(k=513),
    }
    try:
        for name, change in cases.items():
            c = {**ok, **change}
            for entry in ("host", "session"):
                if entry == "session" and name in ("too-many-items", "k-zero", "k-too-large"):
                    continue   # (a session knows its own B)
                pos, cos = np.full(3, 12345, np.uint32), np.full(2, -7, np.int64)
                length, expo = np.full(2, 12345, np.uint32), np.full(DIMB, 12345, np.uint32)
                tail = (p(c["inv"]), p(c["test"][0]), p(c["test"][1]), c["budget"], p(pos), p(cos), p(length), p(expo))
                if entry == "host":
                    rc = lib.poismf_hip_list_eval(p(B), c["k"], c["dimB"], p(c["lists"]), 2, c["n"], *tail)
                else:
                    rc = lib.poismf_hip_session_list_eval(s.h, p(c["lists"]), 2, c["n"], *tail)
                assert rc == 2, (name, entry)
                assert np.all(pos == 12345) and np.all(cos == -7) and np.all(length == 12345) and np.all(expo == 12345), (name, entry)
        pos, cos = np.full(3, 12345, np.uint32), np.full(2, -7, np.int64)
        length, expo = np.full(2, 12345, np.uint32), np.full(DIMB, 12345, np.uint32)
        outs = (p(pos), p(cos), p(length), p(expo))
        null_outs = [(None,) + outs[1:], outs[:1] + (None,) + outs[2:], outs[:2] + (None,) + outs[3:], outs[:3] + (None,)]
        for o in null_outs:
            assert lib.poismf_hip_session_list_eval(s.h, p(ok["lists"]), 2, 3, p(inv), p(ok["test"][0]), p(ok["test"][1]), 0, *o) == 2
        assert lib.poismf_hip_session_list_eval(s.h, None, 2, 3, p(inv), None, None, 0, *outs) == 2
        # no users: 0 whatever else is passed, and nothing is touched -- the exposure counts are not zeroed either
        assert lib.poismf_hip_session_list_eval(s.h, None, 0, 0, None, None, None, 1, *outs) == 0
        assert lib.poismf_hip_list_eval(None, 0, DIMB, None, 0, 0, None, None, None, 1, *outs) == 0
        assert np.all(pos == 12345) and np.all(cos == -7) and np.all(length == 12345) and np.all(expo == 12345)
        assert lib.poismf_hip_session_list_eval(s.h, p(ok["lists"]), 2, 3, p(inv), p(ok["test"][0]), p(ok["test"][1]), 0, *outs) == 0
        assert pos.tolist() == [1, api.LIST_ABSENT, 0] and length.tolist() == [3, 2] and expo.sum() == 5 and np.all(cos != -7)
    finally:
        s.close()
