"""Batched top-N with per-group quotas (include/poismf_hip.h section 1n) on the GPU: items and score bits against a walk of the user's
complete ranked list with one counter per group, over depths, exclusions that move in-group ranks, group schemes (many small groups,
unequal blocks with barred and unconstrained groups, one group for everything), all-tie, short and empty rows; ties across item slices
and at the quota boundary; the reductions to Session.topn_batch; quotas that sum to less than n_top; independence of the batch a user is
in, the host-pointer entry and the R flavour; and the shared scratch left usable.

The expectation is built as in tests/test_gpu_topn_deep.py from Session.predict -- the pair_dot_kernel path, which the batched code does
not share: the user's whole score row, minus E(u), ordered by (score descending, item ascending) with np.lexsort, then walked: an item is
taken iff fewer than quota[g] items of its group were taken, until n are taken; the rest of the row is TOPN_NONE and -inf.  quota_walk is
that walk with explicit counters; quota_select gives the same answer from in-group ranks, vectorised (tests/test_topn_quota_cpu.py holds
both to hand-written answers and to each other).  There is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_topn_deep import DIMA, DIMB, ZERO_USER, FEW_USER, NONE_USER, _excl_pair, _factors, _near_the_top, _score_rows, _session

pytestmark = pytest.mark.gpu

KS = (3, 50, 65)   # 65: two LDS chunks in fp32
DEPTHS = (1, 10, 100, 128)


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


# ---- the reference ----
def ranked(scores, excl):
    """the admissible items of one user in the total order (score descending, item ascending): (items, scores)"""
    idx = np.setdiff1d(np.arange(len(scores)), np.asarray(excl, np.int64))
    s = scores[idx]
    o = np.lexsort((idx, -s.astype(np.float64)))   # (the cast is exact; it only keeps -s in one dtype)
    return idx[o], s[o]


def quota_walk(items, group_of, quota, n):
    """positions (into the ranked list `items`) of the items taken: walk the list, take an item iff fewer than quota[g] items of its
    group were taken, stop at n"""
    taken, count = [], {}
    for p, j in enumerate(items):
        if len(taken) == n:
            break
        g = int(group_of[j])
        if count.get(g, 0) < int(quota[g]):
            count[g] = count.get(g, 0) + 1
            taken.append(p)
    return np.asarray(taken, np.int64)


def quota_select(items, group_of, quota, n):
    """quota_walk's answer from the definition: position p is in Q iff its in-group rank (the earlier positions of its group) is below the
    group's quota; the answer is the first n of Q"""
    g = np.asarray(group_of)[items].astype(np.int64)
    by_group = np.argsort(g, kind="stable")
    gs = g[by_group]
    first = np.r_[0, np.flatnonzero(np.diff(gs)) + 1] if len(gs) else np.empty(0, np.int64)
    rank = np.empty(len(g), np.int64)
    rank[by_group] = np.arange(len(g)) - np.repeat(first, np.diff(np.r_[first, len(g)]))
    q = np.minimum(np.asarray(quota)[g].astype(np.float64), float(len(g) + 1))   # (a quota of 2^31 and more: above every rank)
    return np.flatnonzero(rank < q)[:n]


def expect(lists, group_of, quota, n, dtype, select=quota_select):
    """[m x n] items and scores from the users' ranked lists"""
    ix = np.full((len(lists), n), api.TOPN_NONE, np.uint64)
    sc = np.full((len(lists), n), -np.inf, dtype)
    for i, (items, s) in enumerate(lists):
        p = select(items, group_of, quota, n)
        ix[i, :len(p)] = items[p]
        sc[i, :len(p)] = s[p]
    return ix, sc


def same(got, want, what):
    ok_ix, ok_sc = np.array_equal(got[0], want[0]), got[1].tobytes() == want[1].tobytes()
    print(f"{what}: equal ix {ok_ix} equal score bits {ok_sc}")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    if not ok_ix:
        bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
        raise AssertionError((what, "rows", bad[:8].tolist(), got[0][bad[0]][:12], want[0][bad[0]][:12]))
    assert ok_sc, what


# ---- group schemes: name -> (group_of, quota as a function of n_top) ----
def _blocks():
    """contiguous blocks of 1 .. 600 items; group id 3 is never used; ids 1 and 6 are barred"""
    sizes = [1, 600, 7, 64, 250, 2, 129, 33, 411, 5, 16, 300, 65, 100, 580, 1, 3]
    g, gid, b = [], 0, 0
    while len(g) < DIMB:
        g += [gid] * sizes[b % len(sizes)]
        b += 1
        gid += 2 if gid == 2 else 1
    g = np.asarray(g[:DIMB], np.uint64)
    assert 3 not in g and g.max() > 6
    n_groups = int(g.max()) + 1

    def quota(n):
        q = np.array([(0, 1, 2, n, 2 ** 31)[(i * 7 + 3) % 5] for i in range(n_groups)], np.uint64)
        q[1] = q[6] = 0
        return q
    return g, quota


def _schemes():
    mod = (np.arange(DIMB) % 37).astype(np.uint64)
    blocks, bq = _blocks()
    return {
        "mod37-q1": (mod, lambda n: 1), "mod37-q2": (mod, lambda n: 2), "mod37-q3": (mod, lambda n: 3),
        "blocks": (blocks, bq),
        "one-group-q5": (np.zeros(DIMB, np.uint64), lambda n: 5),
    }


def _quota_array(group_of, q):
    return np.full(int(group_of.max()) + 1, q, np.uint64) if np.ndim(q) == 0 else q


@pytest.mark.parametrize("k", KS)
def test_bits_against_the_walk(prec, k):
    """every depth x {no exclusion, a batch list, exclude_seen, both} x every group scheme; the excluded items come from the top of the
    user's list, so they move in-group ranks; one user keeps 5 items, one keeps none, one row of A is zero"""
    A, B = _factors(DIMA, DIMB, k, prec, 300 + k)
    A[ZERO_USER] = 0
    rng = np.random.default_rng(k)
    seen = _near_the_top(A, B, 2, 200)
    extra = _near_the_top(A, B, 3, 300)
    everything = np.arange(DIMB)
    seen[FEW_USER + 4] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))
    seen[NONE_USER + 4] = everything
    extra[FEW_USER] = np.setdiff1d(everything, rng.choice(DIMB, 5, replace=False))
    extra[NONE_USER] = everything
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, users, DIMB)
        assert not rows[ZERO_USER].any()
        none = [np.empty(0, np.int64)] * DIMA
        both = [np.union1d(a, b) for a, b in zip(seen, extra)]
        lists = {w: [ranked(rows[i], e[i]) for i in range(DIMA)] for w, e in (("plain", none), ("list", extra), ("seen", seen), ("both", both))}
        pair = _excl_pair(extra)
        kwargs = {"plain": {}, "list": {"exclude": pair}, "seen": {"exclude_seen": True}, "both": {"exclude_seen": True, "exclude": pair}}
        schemes = _schemes()

        # the quotas bind: under j % 37 with quota 1 the answer is not the plain top 10 for at least half of the users
        mod = schemes["mod37-q1"][0]
        want10 = expect(lists["plain"], mod, _quota_array(mod, 1), 10, rows.dtype)
        plain10 = np.stack([it[:10] for it, _ in lists["plain"]]).astype(np.uint64)
        differ = int((want10[0] != plain10).any(axis=1).sum())
        print(f"k {k}: the quota changes the top 10 of {differ} of {DIMA} users")
        assert 2 * differ >= DIMA
        # all ties: the smallest admissible indices the quotas allow -- one per group, 0 .. 9
        assert want10[0][ZERO_USER].tolist() == list(range(10))

        for name, (group_of, quota_of) in schemes.items():
            for n in DEPTHS:
                q = quota_of(n)
                qa = _quota_array(group_of, q)
                for w in lists:
                    want = expect(lists[w], group_of, qa, n, rows.dtype)
                    same(s.topn_quota(users, n, group_of=group_of, quota=q, output_score=True, **kwargs[w]), want, f"{name} n {n} {w}")
                    if name == "one-group-q5" and n == 10 and w == "plain":
                        assert np.all(want[0][:, 5:] == api.TOPN_NONE) and np.all(want[0][:, :5] != api.TOPN_NONE)
                    if w == "list":
                        assert (want[0][FEW_USER] != api.TOPN_NONE).sum() <= 5 and (want[0][NONE_USER] == api.TOPN_NONE).all()
        ix, sc = s.topn_quota(users, 10, group_of=mod, quota=1)
        assert np.array_equal(ix, want10[0]) and sc.size == 0
    finally:
        s.close()


def test_the_two_references_agree_on_the_gpu_shapes(prec):
    """quota_select (used above) against the walk with counters, on real score rows"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 5)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        users = np.arange(0, DIMA, 13, dtype=np.uint64)
        rows = _score_rows(s, users, DIMB)
        lists = [ranked(r, [7, 99]) for r in rows]
        for name, (group_of, quota_of) in _schemes().items():
            for n in (10, 128):
                qa = _quota_array(group_of, quota_of(n))
                a, b = expect(lists, group_of, qa, n, rows.dtype), expect(lists, group_of, qa, n, rows.dtype, select=quota_walk)
                assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (name, n)
    finally:
        s.close()


def test_ties_across_slices_and_at_the_quota_boundary(prec):
    """200 rows of B repeated at far-apart indices: the twins tie in score for every user; half of them share their twin's group (at
    quota 1 the smaller index takes the group's slot), half lie in another group.  Few users: many item slices and the merge; 768 x 64
    entries that repeat the 130 rows: one slice, no merge"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 91)
    rng = np.random.default_rng(17)
    src = rng.choice(1400, 200, replace=False)
    dst = src + 1600
    B[dst] = B[src]
    group_of = (np.arange(DIMB) % 37).astype(np.uint64)
    group_of[dst[:100]] = group_of[src[:100]]
    group_of[dst[100:]] = (group_of[src[100:]] + 1) % 37
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, everyone, DIMB)
        assert np.array_equal(rows[:, dst], rows[:, src])
        lists = [ranked(r, []) for r in rows]
        few = np.array([0, 64, 129, 5, 77], np.uint64)
        for n, q in ((10, 1), (100, 2), (128, 5)):
            want = expect(lists, group_of, _quota_array(group_of, q), n, rows.dtype)
            got = s.topn_quota(few, n, group_of=group_of, quota=q, output_score=True)
            same(got, (want[0][few.astype(np.int64)], want[1][few.astype(np.int64)]), f"few users n {n} q {q}")
            same(s.topn_quota(everyone, n, group_of=group_of, quota=q, output_score=True), want, f"130 users n {n} q {q}")
        # twins of one group meet at the boundary: both in a user's plain top 10, only the smaller index in the quota's answer
        want = expect(lists, group_of, _quota_array(group_of, 1), 10, rows.dtype)
        met = sum(1 for i, (it, _) in enumerate(lists) for a, b in zip(src[:100], dst[:100])
                  if a in it[:10] and b in it[:10] and a in want[0][i] and b not in want[0][i])
        print(f"twins of one group at the boundary: {met}")
        assert met > 0
        many = np.tile(everyone, 768 * 64 // DIMA + 1)[:768 * 64]
        ix, sc = s.topn_quota(many, 10, group_of=group_of, quota=1, output_score=True)
        same((ix[:DIMA], sc[:DIMA]), want, "one slice")
        m = many.astype(np.int64)
        assert np.array_equal(ix, ix[:DIMA][m]) and sc.tobytes() == sc[:DIMA][m].tobytes()   # every repeat equals the first occurrence
    finally:
        s.close()


def test_reductions_to_the_plain_call(prec):
    """bit for bit Session.topn_batch on the same session: every quota >= n_top; every item its own group at quota 1; quota 0 on some
    groups against topn_batch with those groups' items excluded"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 23)
    seen = _near_the_top(A, B, 2, 100)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        mod = (np.arange(DIMB) % 37).astype(np.uint64)
        own = np.arange(DIMB, dtype=np.uint64)
        barred = np.flatnonzero(np.isin(mod, (0, 5, 36)))
        q0 = np.full(37, 2 ** 31, np.uint64)
        q0[[0, 5, 36]] = 0
        pair = _excl_pair([barred] * DIMA)                      # (n_top items remain for everyone: 249 of 3077 are barred, 50 seen)
        for n in (1, 10, 128):
            plain = s.topn_batch(users, n, exclude_seen=True, output_score=True)
            for what, got in (("quota = n_top", s.topn_quota(users, n, group_of=mod, quota=n, exclude_seen=True, output_score=True)),
                              ("quota above n_top", s.topn_quota(users, n, group_of=mod, quota=2 ** 40, exclude_seen=True, output_score=True)),
                              ("own group", s.topn_quota(users, n, group_of=own, quota=1, exclude_seen=True, output_score=True))):
                same(got, plain, f"{what} n {n}")
            same(s.topn_quota(users, n, group_of=mod, quota=q0, exclude_seen=True, output_score=True),
                 s.topn_batch(users, n, exclude_seen=True, exclude=pair, output_score=True), f"quota 0 n {n}")
    finally:
        s.close()


def test_quotas_that_sum_to_less_than_n_top(prec):
    """3 groups at quota 1 and n_top 10: three entries and seven pads (the slow path: the threshold never rises, so only at this shape)"""
    k = 8
    A, B = _factors(DIMA, DIMB, k, prec, 61)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        group_of = (np.arange(DIMB) % 3).astype(np.uint64)
        lists = [ranked(r, [u % DIMB]) for u, r in enumerate(_score_rows(s, users, DIMB))]
        want = expect(lists, group_of, np.ones(3, np.uint64), 10, H.dtype_of(prec))
        assert np.all(want[0][:, :3] != api.TOPN_NONE) and np.all(want[0][:, 3:] == api.TOPN_NONE) and np.all(want[1][:, 3:] == -np.inf)
        same(s.topn_quota(users, 10, group_of=group_of, quota=1, exclude_seen=True, output_score=True), want, "sum of quotas 3")
        zero = s.topn_quota(users, 10, group_of=group_of, quota=0, output_score=True)
        assert np.all(zero[0] == api.TOPN_NONE) and np.all(zero[1] == -np.inf)
    finally:
        s.close()


def test_independence_host_pointers_and_the_r_flavour(prec):
    """a user alone, in a shuffled batch and in a batch with repeats: the same row; PoisMF.topN_quota (host pointers) and, in double, the
    R flavour through ctypes: the session's rows, bit for bit"""
    k, n = 50, 20
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    seen = _near_the_top(A, B, 2, 200)
    s = _session(DIMA, DIMB, k, prec, A, B, seen)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    group_of, bq = _blocks()
    quota = bq(n)
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        call = lambda u: s.topn_quota(u, n, group_of=group_of, quota=quota, exclude_seen=True, output_score=True)
        ix_all, sc_all = call(everyone)
        perm = np.random.default_rng(3).permutation(DIMA)
        ix_p, sc_p = call(everyone[perm])
        assert np.array_equal(ix_p, ix_all[perm]) and sc_p.tobytes() == sc_all[perm].tobytes()
        for u in (0, 63, 64, 129):
            ix1, sc1 = call([u])
            ix3, sc3 = call([u, 11, u, 100, u])
            for p in (0, 2, 4):
                assert np.array_equal(ix3[p], ix_all[u]) and sc3[p].tobytes() == sc_all[u].tobytes()
            assert np.array_equal(ix1[0], ix_all[u]) and sc1[0].tobytes() == sc_all[u].tobytes()
        users = np.array([3, 129, 64, 3, 77, 0], np.uint64)
        pair = _excl_pair([seen[u] for u in users])
        a = call(users)
        b = m.topN_quota(users, n, group_of=group_of, quota=quota, exclude=pair, output_score=True)   # (the batch's rows of A only)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        pair_all = _excl_pair(seen)
        c = m.topN_quota(everyone, n, group_of=group_of, quota=quota, exclude=pair_all, output_score=True)   # (all of A goes up)
        assert np.array_equal(c[0], ix_all) and c[1].tobytes() == sc_all.tobytes()
        if not prec:
            lib = api.load_library("r")
            i32 = lambda v: np.ascontiguousarray(np.minimum(np.asarray(v, np.uint64), 2 ** 31 - 1).astype(np.int32))
            u, g, q, ip, ii = i32(everyone), i32(group_of), i32(quota), i32(pair_all[0]), i32(pair_all[1])
            out, sc = np.zeros((DIMA, n), np.int32), np.zeros((DIMA, n), np.float64)
            p = api._ptr
            rc = lib.poismf_hip_topn_quota(p(A), p(B), k, DIMA, DIMB, p(u), DIMA, n, p(g), len(q), p(q), p(ip), p(ii), p(out), p(sc))
            assert rc == 0
            wide = np.where(out < 0, np.uint64(api.TOPN_NONE), out.astype(np.int64).astype(np.uint64))
            assert np.array_equal(out < 0, ix_all == api.TOPN_NONE)      # (the R flavour's TOPN_NONE is -1)
            assert np.array_equal(wide, ix_all) and sc.tobytes() == sc_all.tobytes()
    finally:
        s.close()


def test_the_session_is_left_as_it_was(prec):
    """topn_batch before and after a quota call gives the same rows (the calls share the session's scratch), and so does a second quota
    call after a deep one has grown it"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 8)
    s = _session(DIMA, DIMB, k, prec, A, B)
    try:
        users = np.arange(DIMA, dtype=np.uint64)
        mod = (np.arange(DIMB) % 37).astype(np.uint64)
        before = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
        first = s.topn_quota(users, 10, group_of=mod, quota=2, exclude_seen=True, output_score=True)
        after = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
        assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()
        s.topn_deep(users, 1024)
        second = s.topn_quota(users, 10, group_of=mod, quota=2, exclude_seen=True, output_score=True)
        assert np.array_equal(first[0], second[0]) and first[1].tobytes() == second[1].tobytes()
    finally:
        s.close()
