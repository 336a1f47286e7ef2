"""The serving calls (include/poismf_hip.h sections 1d, 1f - 1p) on the GPU against an expectation that holds no GPU code, on the inputs
the rest of the suite never draws: negative scores, thousands of exact ties, rows of zeros, subnormal operands and results, huge scores
and infinite ones (tests/serving_values.py; tests/test_serving_values_cpu.py shows that its integer scores are exact in real_t in every
summation order).  One session per (regime, precision, k) on 150 users x 3077 items -- two full tiles of users and a part of a third,
48 full tiles of items and one with 59 phantom columns -- built from a small COO so that exclude_seen has resident rows.

Every comparison is on indices and on score bits; there is no tolerance in this file.  Next to the general comparison each regime
asserts what it is there to catch, so that a failure reads as its cause:
    signed    user 1's scores are all negative: a phantom column (score 0) would head its lists and add to every rank
    sparse    user 0's scores are all 0: its answer is the first admissible indices
    sub_*     the tile's engine and the scalar chains agree on subnormals: a held-out item never comes before itself
    overflow  +inf items first and -inf items last, each by index, and none missing: user 3 keeps exactly 128 items, some at -inf
"""
import numpy as np
import pytest

from poismf_amd import api
from tests import serving_values as V
from tests.test_gpu_topn_quota import expect as quota_expect, quota_select
from tests.test_gpu_topn_weighted import weighted_expect

pytestmark = pytest.mark.gpu

EVERYONE = np.arange(V.DIMA, dtype=np.uint64)
FIXED = np.arange(4, dtype=np.uint64)            # few users: many item slices and the merge kernels
SOME = np.r_[0:4, np.random.default_rng(5).choice(np.arange(4, V.DIMA), 16, replace=False)].astype(np.uint64)


def _session(param):
    w = V.world(*param)
    s = api.Session.from_coo(w.coo(), w.k, w.is_float)
    try:
        s.set_factors(w.A, w.B)
        yield w, s
    finally:
        s.close()


@pytest.fixture(scope="module", params=V.CASES, ids=V.case_id)
def case(request):
    yield from _session(request.param)


# sections 1o and 1p leave denormal products unspecified, and a weight times an infinity is outside their contract: the calls that
# multiply a score run in the regimes whose scores are plain integers
@pytest.fixture(scope="module", params=[c for c in V.CASES if c[0] in ("signed", "sparse")], ids=V.case_id)
def product_case(request):
    yield from _session(request.param)


def _name(w):
    return V.case_id((w.regime, w.is_float, w.k))


def _same(w, entry, users, got, want):
    """items and score bits of got == want, row by row; the message names the regime, precision, k, entry point and user"""
    (ix, sc), (eix, esc) = got, want
    assert ix.shape == eix.shape and sc.shape == esc.shape and sc.dtype == esc.dtype, (_name(w), entry, ix.shape, eix.shape, sc.shape, esc.shape)
    bad = np.flatnonzero((ix != eix).any(axis=1) | (V.bits(sc) != V.bits(esc)).any(axis=1))
    print(f"{_name(w)} {entry}: {len(users)} rows, {len(bad)} differ")
    if len(bad):
        i = int(bad[0])
        c = np.flatnonzero((ix[i] != eix[i]) | (V.bits(sc[i]) != V.bits(esc[i])))[:8]
        raise AssertionError(f"{_name(w)} {entry}: user {int(users[i])} (row {i}; {len(bad)} rows differ), columns {c.tolist()}: "
                             f"items {ix[i, c].tolist()} expected {eix[i, c].tolist()}, scores {sc[i, c].tolist()} expected {esc[i, c].tolist()}")


def _regime(w, entry, users, got, mask, n):
    """what each regime is there to catch, on the rows of one top-N call over the admissible sets `mask`"""
    ix, sc = got
    for i, u in enumerate(users):
        u = int(u)
        adm = np.flatnonzero(mask[i])
        full = min(n, len(adm))
        where = f"{_name(w)} {entry}: user {u}"
        if w.regime == "signed" and u == 1:
            assert (ix[i, :full] < V.DIMB).all() and mask[i, ix[i, :full].astype(np.int64)].all() and (sc[i, :full] < 0).all(), \
                f"{where}: a list of negative scores holds something that is no admissible item (a phantom column scores 0)"
        if w.regime == "sparse" and u == 0:
            assert np.array_equal(ix[i, :full], adm[:full].astype(np.uint64)) and not sc[i, :full].any(), \
                f"{where}: among scores of 0 the answer is the first admissible indices"
        if w.regime == "overflow" and w.sign0[u]:
            up, down = adm[np.isposinf(w.S[u, adm])], adm[np.isneginf(w.S[u, adm])]
            head = min(full, len(up))
            assert np.array_equal(ix[i, :head], up[:head].astype(np.uint64)), f"{where}: the +inf items come first, by index"
            if len(down) and n >= len(adm):
                assert np.array_equal(ix[i, len(adm) - len(down):len(adm)], down.astype(np.uint64)), \
                    f"{where}: the -inf items end the list, by index, and none is missing"
                assert np.isneginf(sc[i, len(adm) - len(down):]).all()


def _topn(w, s, entry, users, n, call, include=None, exclude=None):
    mask = w.mask(users, include=include, exclude=exclude)
    got = call()
    want = w.topn(users, mask, n)
    try:
        _regime(w, f"{entry} n {n}", users, got, mask, n)
    finally:
        _same(w, f"{entry} n {n}", users, got, want)


def _rows(rows, users):
    return [rows[int(u)] for u in users]


def test_predict(case):
    """Session.predict and predict_multiple over whole score rows of the fixed users and 16 others"""
    w, s = case
    iu, ii = np.repeat(SOME, V.DIMB), np.tile(np.arange(V.DIMB, dtype=np.uint64), len(SOME))
    want = w.S[SOME.astype(np.int64)]
    host = np.empty(len(iu), w.dt)
    api._predict_multiple(host, w.A, w.B, iu, ii)
    for entry, got in (("Session.predict", s.predict(iu, ii)), ("predict_multiple", host)):
        got = got.reshape(want.shape)
        bad = np.argwhere(V.bits(got) != V.bits(want))
        print(f"{_name(w)} {entry}: {got.size} scores, {len(bad)} differ")
        if len(bad):
            i, j = bad[0]
            raise AssertionError(f"{_name(w)} {entry}: user {int(SOME[i])} item {j}: {got[i, j]!r} ({V.bits(got)[i, j]:#x}) expected "
                                 f"{want[i, j]!r} ({V.bits(want)[i, j]:#x}); {len(bad)} scores differ")


def test_topn_of_one_user(case):
    """Session.topn and the drop-in topN: plain, over an include list, minus an exclude list (user 3: down to its last admissible item)"""
    w, s = case
    none = np.empty(0, np.uint64)
    for u in (0, 1, 2, 3, 5, 64, 149):
        row = np.array([u], np.uint64)
        inc, exc = w.incl[u].astype(np.uint64), w.extra[u].astype(np.uint64)
        calls = [("plain", 10, none, none), ("plain", 128, none, none), ("include", min(10, len(inc)), inc, none),
                 ("include", len(inc) if len(inc) <= 65 else 128, inc, none), ("exclude", 10, none, exc),
                 ("exclude", 128 if u == 3 else 77, none, exc)]
        for how, n, i_, e_ in calls:
            if n == 0 or (how == "exclude" and len(e_) == 0):
                continue
            kw = dict(include=[i_.astype(np.int64)] if len(i_) else None, exclude=[e_.astype(np.int64)] if len(e_) else None)
            def one(call):
                ix, sc = call()
                return ix.reshape(1, n), sc.reshape(1, n)
            _topn(w, s, f"Session.topn {how}", row, n, lambda: one(lambda: s.topn(u, n, i_, e_, output_score=True)), **kw)
            _topn(w, s, f"topN {how}", row, n, lambda: one(lambda: api._call_topN(w.A[u].copy(), w.B, i_, e_, n, 1)), **kw)


@pytest.mark.parametrize("users", [EVERYONE, FIXED], ids=["all-users", "fixed-users"])
def test_topn_batch(case, users):
    """plain, exclude_seen, an exclusion list, both; user 3 keeps exactly 128 items under its list"""
    w, s = case
    seen, extra, both = _rows(w.seen, users), _rows(w.extra, users), _rows(w.both, users)
    pair = w.pair(w.extra, users)
    for n in (1, 10, 128):
        _topn(w, s, "topn_batch plain", users, n, lambda: s.topn_batch(users, n, output_score=True))
        _topn(w, s, "topn_batch exclude_seen", users, n, lambda: s.topn_batch(users, n, exclude_seen=True, output_score=True), exclude=seen)
        _topn(w, s, "topn_batch exclude=", users, n, lambda: s.topn_batch(users, n, exclude=pair, output_score=True), exclude=extra)
        _topn(w, s, "topn_batch both", users, n, lambda: s.topn_batch(users, n, exclude_seen=True, exclude=pair, output_score=True), exclude=both)


def test_topn_batch_include(case):
    """a list per user of 0, 1, 5, 64, 65 and 700 items, some in the last tile; short rows come back padded"""
    w, s = case
    users = EVERYONE
    incl, both = _rows(w.incl, users), _rows(w.both, users)
    ipair, epair = w.pair(w.incl, users), w.pair(w.extra, users)
    for n in (1, 10, 128):
        _topn(w, s, "topn_batch include=", users, n, lambda: s.topn_batch(users, n, include=ipair, output_score=True), include=incl)
        _topn(w, s, "topn_batch include= both", users, n,
              lambda: s.topn_batch(users, n, include=ipair, exclude_seen=True, exclude=epair, output_score=True), include=incl, exclude=both)
    if w.regime == "overflow":
        ix, _ = s.topn_batch(users, 10, include=ipair, output_score=True)
        for u in range(V.DIMA):
            if 0 < len(w.incl[u]) <= 5:
                assert sorted(ix[u, :len(w.incl[u])].tolist()) == w.incl[u].tolist(), f"{_name(w)} include=: user {u}'s short list is not complete"


def test_topn_batch_shared(case):
    """three lists shared between users, one of them all items"""
    w, s = case
    users = EVERYONE
    table = V._csr_pair(w.shared)
    incl, both = [w.shared[int(g)] for g in w.shared_of], _rows(w.both, users)
    epair = w.pair(w.extra, users)
    for n in (10, 128):
        _topn(w, s, "topn_batch include_of=", users, n,
              lambda: s.topn_batch(users, n, include=table, include_of=w.shared_of, output_score=True), include=incl)
        _topn(w, s, "topn_batch include_of= both", users, n,
              lambda: s.topn_batch(users, n, include=table, include_of=w.shared_of, exclude_seen=True, exclude=epair, output_score=True),
              include=incl, exclude=both)


@pytest.mark.parametrize("n", [300, 1024])
def test_topn_deep(case, n):
    """deep lists; user 3 (128 items left) and, at 1024, nobody's padding may hold a phantom"""
    w, s = case
    for users in (EVERYONE, FIXED):
        extra, both = _rows(w.extra, users), _rows(w.both, users)
        pair = w.pair(w.extra, users)
        _topn(w, s, f"topn_deep plain {len(users)} users", users, n, lambda: s.topn_deep(users, n, output_score=True))
        _topn(w, s, f"topn_deep exclude= {len(users)} users", users, n, lambda: s.topn_deep(users, n, exclude=pair, output_score=True), exclude=extra)
        _topn(w, s, f"topn_deep both {len(users)} users", users, n,
              lambda: s.topn_deep(users, n, exclude_seen=True, exclude=pair, output_score=True), exclude=both)


def test_topn_quota(case):
    """groups j % 7: quota 2 (rows padded from 14 on) and quota = n (section 1f's rows)"""
    w, s = case
    group_of = np.arange(V.DIMB) % 7
    for users in (EVERYONE, FIXED):
        both = _rows(w.both, users)
        pair = w.pair(w.extra, users)
        mask = w.mask(users, exclude=both)
        lists = []
        for i, u in enumerate(users):
            o = w.order[int(u)]
            o = o[mask[i, o]]
            lists.append((o, w.S[int(u), o]))
        for n, q in ((10, 2), (128, 2), (10, 10), (128, 128)):
            want = quota_expect(lists, group_of, np.full(7, q), n, w.dt, select=quota_select)
            got = s.topn_quota(users, n, group_of=group_of, quota=q, exclude_seen=True, exclude=pair, output_score=True)
            entry = f"topn_quota quota {q} n {n} {len(users)} users"
            if q == n:
                _regime(w, entry, users, got, mask, n)
            _same(w, entry, users, got, want)


def test_topn_weighted(product_case):
    """integer weights in {0, 1, 2, 3}: the products stay exact.  A negative score times a weight of 0 is -0, in the expectation as on the
    device ("bit for bit predict_multiple's score multiplied by item_weight[j]", section 1o), and it ties with +0 by index."""
    w, s = product_case
    weight = np.random.default_rng(9).integers(0, 4, V.DIMB).astype(w.dt)
    for users in (EVERYONE, FIXED):
        both = _rows(w.both, users)
        pair = w.pair(w.extra, users)
        rows = w.S[users.astype(np.int64)]
        for n in (10, 128):
            eix, esc = weighted_expect(rows, weight, both, n)
            got = s.topn_weighted(users, n, item_weight=weight, exclude_seen=True, exclude=pair, output_score=True)
            _same(w, f"topn_weighted n {n} {len(users)} users", users, got, (eix, esc))
        if w.regime == "sparse" and 0 in users:
            adm = np.flatnonzero(w.mask(users[:1], exclude=both[:1])[0])
            assert np.array_equal(got[0][0], adm[:128].astype(np.uint64)), f"{_name(w)} topn_weighted: user 0's answer is the first admissible indices"


def test_topn_diverse_at_lambda_one(product_case):
    """lam = 1 is pure relevance: topn_deep's first n, items and scores"""
    w, s = product_case
    n2 = (w.Bi * w.Bi).sum(axis=1).astype(w.dt)
    for users in (EVERYONE, FIXED):
        both = _rows(w.both, users)
        pair = w.pair(w.extra, users)
        for n, pool in ((10, 100), (128, 300)):
            ix, sc, _ = s.topn_diverse(users, n, pool, 1.0, exclude_seen=True, exclude=pair, output_score=True, item_norm=n2)
            _topn(w, s, f"topn_diverse lam 1 pool {pool} {len(users)} users", users, n, lambda: (ix, sc), exclude=both)


def _ranks(w, s, entry, users, call, topn, include=None, exclude=None, unite=None):
    tests = _rows(w.test, users)
    mask = w.mask(users, include=include, exclude=exclude, unite=unite)
    (ranks, n_adm), (eranks, en_adm) = call(), w.ranks(users, mask, tests)
    ranks, eranks = ranks.reshape(len(users), V.N_TEST), eranks.reshape(len(users), V.N_TEST)
    bad = np.flatnonzero((ranks != eranks).any(axis=1) | (n_adm != en_adm))
    print(f"{_name(w)} {entry}: {ranks.size} cells, rows that differ {len(bad)}")
    # a held-out item stands in the same call's top-N at its rank: it never comes before itself, whatever engine scored it
    if topn is not None:
        ix, n = topn()[0], 128
        for i in range(len(users)):
            for t, r in zip(tests[i], ranks[i]):
                if r < n:
                    assert ix[i, r] == t, (f"{_name(w)} {entry}: user {int(users[i])} item {int(t)} has rank {int(r)}, where the top-N of the same "
                                           f"exclusions lists item {int(ix[i, r])}")
    if len(bad):
        i = int(bad[0])
        hint = " (a phantom column would add 59 per slice of items)" if w.regime == "signed" and int(users[i]) == 1 else ""
        raise AssertionError(f"{_name(w)} {entry}: user {int(users[i])} ({len(bad)} rows differ){hint}: held-out items {tests[i].tolist()} ranks "
                             f"{ranks[i].tolist()} expected {eranks[i].tolist()}, admissible {int(n_adm[i])} expected {int(en_adm[i])}")


def test_rank_batch(case):
    """12 held-out items per user, some excluded, some of J: against the whole catalogue, a list per user, and shared lists united with
    the held-out rows"""
    w, s = case
    for users in (EVERYONE, FIXED):
        tpair, epair, ipair = w.pair(w.test, users), w.pair(w.extra, users), w.pair(w.incl, users)
        extra, both, incl = _rows(w.extra, users), _rows(w.both, users), _rows(w.incl, users)
        tag = f"{len(users)} users"
        _ranks(w, s, f"rank_batch plain {tag}", users, lambda: s.rank_batch(users, tpair), lambda: s.topn_batch(users, 128))
        _ranks(w, s, f"rank_batch exclude= {tag}", users, lambda: s.rank_batch(users, tpair, exclude=epair),
               lambda: s.topn_batch(users, 128, exclude=epair), exclude=extra)
        _ranks(w, s, f"rank_batch both {tag}", users, lambda: s.rank_batch(users, tpair, exclude_seen=True, exclude=epair),
               lambda: s.topn_batch(users, 128, exclude_seen=True, exclude=epair), exclude=both)
        _ranks(w, s, f"rank_batch include= {tag}", users, lambda: s.rank_batch(users, tpair, include=ipair, exclude_seen=True, exclude=epair),
               lambda: s.topn_batch(users, 128, include=ipair, exclude_seen=True, exclude=epair), include=incl, exclude=both)
        table, of = V._csr_pair(w.shared), w.shared_of[users.astype(np.int64)]
        shared = [w.shared[int(g)] for g in of]
        _ranks(w, s, f"rank_batch include_of= {tag}", users,
               lambda: s.rank_batch(users, tpair, include=table, include_of=of, exclude_seen=True, exclude=epair),
               lambda: s.topn_batch(users, 128, include=table, include_of=of, exclude_seen=True, exclude=epair), include=shared, exclude=both)
        _ranks(w, s, f"rank_batch include_of= unite_test {tag}", users,
               lambda: s.rank_batch(users, tpair, include=table, include_of=of, unite_test=True, exclude_seen=True, exclude=epair),
               None, include=shared, exclude=both, unite=_rows(w.test, users))


@pytest.mark.parametrize("regime", V.REGIMES)
def test_host_pointer_entry(regime):
    """PoisMF.topN_batch: the factors go up from the host"""
    w = V.world(regime, True, 50)
    m = api.PoisMF(k=w.k, use_float=True)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = w.A, w.B, V.DIMA, V.DIMB, True
    users = EVERYONE
    pair, extra = w.pair(w.extra, users), _rows(w.extra, users)
    for n in (10, 128):
        _topn(w, None, "PoisMF.topN_batch", users, n, lambda: m.topN_batch(users, n, exclude=pair, output_score=True), exclude=extra)
    ipair = w.pair(w.incl, users)
    _topn(w, None, "PoisMF.topN_batch include=", users, 10, lambda: m.topN_batch(users, 10, include=ipair, output_score=True), include=_rows(w.incl, users))
