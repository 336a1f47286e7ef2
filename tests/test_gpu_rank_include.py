"""Batched exact ranks among per-user include lists (include/poismf_hip.h section 1j) on the GPU: ranks and admissible counts against
the existing predict path, equivalence with the dense call of section 1g given the complement, agreement with the batched top-N
over the same lists, ties, independence of the batch a user is in (a batch cut into chunks included), empty and wholly excluded
lists, the entry points against each other, and the argument checks on a machine that has a device.

The expectation is built from Session.predict -- the pair_dot_kernel path: the user's whole score row restricted to I(u) \\ E(u),
ordered by (score descending, item ascending) with np.lexsort; a held-out item's rank is its position in that list.  Every
comparison of ranks is np.array_equal on integers, and no user or cell is left out.

Shapes: 300 users x 3077 items (three slices of a list and a bit); one batch entry for every include-list length 0..200, S - 1, S,
S + 1, 2 S + 1 (S: the slice length) and the whole catalogue; held-out rows of 0, 1, G, G + 1 and 2 G + 1 cells (G: the thresholds
a wave keeps in LDS) among random short ones."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, metrics
from tests import helpers as H
from tests.test_gpu_topn_batch import KS, _excl_pair, _factors, _rows_of, _score_rows, _session
from tests.test_rank_include_cpu import BAD, NO_ROW_COUNT, OK_I, OK_T, _c_call

pytestmark = pytest.mark.gpu

DIMA, DIMB = 300, 3077
S, G = api.RANK_INCLUDE_SLICE, api.RANK_INCLUDE_GROUP
EXCL = api.RANK_EXCLUDED
LENGTHS = list(range(201)) + [S - 1, S, S + 1, 2 * S + 1, DIMB]
HELD = {S - 1: 0, 0: 3, 1: 1, S: G, 2 * S + 1: G + 1, DIMB: 2 * G + 1, S + 1: 2 * G + 40}   # include length -> held-out cells drawn from the list


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


@functools.lru_cache(maxsize=None)
def _matrix():
    """300 x 3077 with ~30 nonzeros per row; SciPy COO with float64 counts"""
    rng = np.random.default_rng(3)
    nnz = 30 * DIMA
    return sp.coo_matrix((np.ones(nnz), (rng.integers(0, DIMA, nnz), rng.integers(0, DIMB, nnz))), shape=(DIMA, DIMB))


@functools.lru_cache(maxsize=None)
def _csr():
    csr = sp.csr_matrix(_matrix())
    csr.sum_duplicates(); csr.sort_indices()
    return csr


@functools.lru_cache(maxsize=None)
def _plan(seed=0):
    """The batch, built once and never changed: users (207 entries, the last repeats the first), their seen rows, extra exclusions,
    include lists (one per length of LENGTHS; the repeat has a list of its own) and held-out rows -- cells from the list, from
    the user's seen row, from its extra exclusions and from outside its list."""
    rng = np.random.default_rng(seed)
    users = rng.permutation(DIMA)[:len(LENGTHS)]
    users = np.concatenate((users, users[:1]))
    lengths = LENGTHS + [150]
    seen = _rows_of(_csr(), users)
    extra = [np.union1d(rng.choice(DIMB, int(rng.integers(0, 40)), replace=False), s[:3]) for s in seen]   # (overlaps the seen row)
    lists, held = [], []
    for i, n in enumerate(lengths):
        first = np.concatenate((seen[i][:4], extra[i][:3], rng.permutation(DIMB)))      # some seen and excluded items are listed
        _, at = np.unique(first, return_index=True)
        lst = np.sort(first[np.sort(at)][:n]).astype(np.int64)
        lists.append(lst)
        if i < len(LENGTHS) and n in HELD:
            t = rng.choice(lst, min(HELD[n], len(lst)), replace=False) if len(lst) else np.empty(0, np.int64)
            if n == 0:
                t = rng.choice(DIMB, HELD[n], replace=False)                             # an empty list: every cell is unlisted
        else:
            own = rng.choice(lst, min(len(lst), int(rng.integers(0, 8))), replace=False) if len(lst) else np.empty(0, np.int64)
            t = np.concatenate((own, rng.choice(DIMB, int(rng.integers(0, 4)), replace=False), seen[i][:2], extra[i][:2]))
        held.append(np.unique(t).astype(np.int64))
    assert len(users) % 64 != 0 and [len(x) for x in lists] == lengths
    assert {0, 1, G, G + 1, 2 * G + 1} <= {len(t) for t in held}
    return users.astype(np.uint64), seen, extra, lists, held


def _cases(seen, extra):
    """the four exclusion cases of a batch: name -> (exclude_seen, list or None, E(u) per user)"""
    none = [np.empty(0, np.int64)] * len(seen)
    both = [np.union1d(a, b) for a, b in zip(seen, extra)]
    return {"plain": (False, None, none), "seen": (True, None, seen), "list": (False, _excl_pair(extra), extra),
            "both": (True, _excl_pair(extra), both)}


def _expect(score_row, lst, excluded, held_out):
    """(ranks of held_out, EXCL where not in I \\ E; N): positions in the lexsort of the admissible candidates"""
    idx = np.setdiff1d(np.asarray(lst, np.int64), np.asarray(excluded, np.int64))
    sc = score_row[idx]
    o = np.lexsort((idx, -sc.astype(np.float64)))          # (the cast is exact; it only keeps -sc in one dtype)
    place = np.full(len(score_row), EXCL, np.int64)
    place[idx[o]] = np.arange(len(idx))
    return place[np.asarray(held_out, np.int64)].astype(np.uint32), len(idx)


def _expect_all(rows, lists, excl, held):
    want = [_expect(rows[i], lists[i], excl[i], held[i]) for i in range(len(lists))]
    return (np.concatenate([w[0] for w in want]) if want else np.empty(0, np.uint32)), np.array([w[1] for w in want], np.uint32)


def _assert_ranks(got, want, held, what):
    ranks, n_adm = got
    assert ranks.dtype == np.uint32 and n_adm.dtype == np.uint32
    assert len(ranks) == len(want[0]) == sum(len(t) for t in held) and len(n_adm) == len(want[1])
    bad_n = np.flatnonzero(n_adm != want[1])
    bad_r = np.flatnonzero(ranks != want[0])
    print(f"{what}: {len(ranks)} cells, {int((want[0] == EXCL).sum())} marked; wrong ranks {len(bad_r)}, wrong N {len(bad_n)}")
    assert len(bad_n) == 0, (what, bad_n[:10], n_adm[bad_n[:10]], want[1][bad_n[:10]])
    assert len(bad_r) == 0, (what, bad_r[:10], ranks[bad_r[:10]], want[0][bad_r[:10]])


def _split(ranks, held):
    at = np.concatenate(([0], np.cumsum([len(t) for t in held])))
    return [ranks[at[i]:at[i + 1]] for i in range(len(held))]


BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_exact_ranks_against_the_predict_path(prec, k):
    """1. out_rank equals each held-out item's position in the lexsort of Session.predict's scores over I(u) \\ E(u); out_n_adm its length"""
    users, seen, extra, lists, held = _plan()
    A, B = _factors(DIMA, DIMB, k, prec, 10 + k)
    s = _session(_matrix(), k, prec, A, B)
    try:
        rows = _score_rows(s, users, DIMB)
        for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
            got = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(lists))
            want = _expect_all(rows, lists, excl, held)
            _assert_ranks(got, want, held, what)
            # the sentinel is exercised for both reasons: a listed item that is excluded, and an unlisted one
            per = _split(got[0], held)
            unlisted = any((r[~np.isin(t, l)] == EXCL).all() and (~np.isin(t, l)).any() for r, t, l in zip(per, held, lists))
            assert unlisted
            if what != "plain":
                assert any((r[np.isin(t, l) & np.isin(t, e)] == EXCL).all() and (np.isin(t, l) & np.isin(t, e)).any()
                           for r, t, l, e in zip(per, held, lists, excl))
    finally:
        s.close()


def test_equivalence_with_the_dense_call(prec):
    """2. section 1g with E(u) united with the complement of I(u) as the exclusion list: identical ranks and N"""
    users, seen, extra, lists, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 21)
    s = _session(_matrix(), k, prec, A, B)
    try:
        everything = np.arange(DIMB)
        for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
            got = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(lists))
            e_rows = extra if lst is not None else [np.empty(0, np.int64)] * len(users)
            dense_excl = [np.union1d(e, np.setdiff1d(everything, l)) for e, l in zip(e_rows, lists)]
            dense = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=_excl_pair(dense_excl))
            assert np.array_equal(got[0], dense[0]), what
            assert np.array_equal(got[1], dense[1]), what
    finally:
        s.close()


def test_agreement_with_topn_include(prec):
    """3. every cell with rank below 128 sits at topn_batch(include=, top_n=128)[u][rank], every listed held-out item has its index as
    its rank, and a padded tail is 128 - N long"""
    users, seen, extra, lists, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 22)
    s = _session(_matrix(), k, prec, A, B)
    try:
        listed = 0
        for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
            ranks, n_adm = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(lists))
            top, _ = s.topn_batch(users, 128, exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(lists))
            for i, r in enumerate(_split(ranks, held)):
                r = r.astype(np.int64)
                low = r < 128
                assert np.array_equal(top[i][r[low]].astype(np.int64), held[i][low]), (what, i)
                where = {int(j): pos for pos, j in enumerate(top[i]) if j != api.TOPN_NONE}
                for t, rt in zip(held[i], r):
                    if int(t) in where:
                        listed += 1
                        assert where[int(t)] == rt, (what, i, int(t), where[int(t)], rt)
                pad = int((top[i] == api.TOPN_NONE).sum())
                assert pad == max(128 - int(n_adm[i]), 0), (what, i, pad, int(n_adm[i]))
                if pad:
                    assert (top[i][128 - pad:] == api.TOPN_NONE).all()
        assert listed > 1000                           # (the comparison is not vacuous)
    finally:
        s.close()


@pytest.mark.parametrize("k", [5, 50])
def test_ties(prec, k):
    """4. 37 distinct rows of B repeated down the catalogue and two zero columns: many equal scores; ranks still equal the lexsort,
    and a held-out item never comes before itself (its rank is below N)"""
    users, seen, extra, lists, held = _plan()
    A, B = _factors(DIMA, DIMB, k, prec, 23)
    B = np.ascontiguousarray(B[np.arange(DIMB) % 37])
    B[:, :2] = 0
    s = _session(_matrix(), k, prec, A, B)
    try:
        rows = _score_rows(s, users, DIMB)
        assert len(np.unique(rows[0])) <= 37
        for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
            got = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(lists))
            _assert_ranks(got, _expect_all(rows, lists, excl, held), held, what)
            for r, n in zip(_split(got[0], held), got[1]):
                assert (r[r != EXCL] < n).all()
    finally:
        s.close()


def test_independence_of_company(prec):
    """5. a user's ranks alone, in the batch, in the reversed batch, and in a batch whose include lists exceed what one chunk of the
    scratch carries: identical"""
    users, seen, extra, lists, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 24)
    s = _session(_matrix(), k, prec, A, B)
    try:
        ranks, n_adm = s.rank_batch(users, _excl_pair(held), exclude_seen=True, exclude=_excl_pair(extra), include=_excl_pair(lists))
        per = _split(ranks, held)
        rev = slice(None, None, -1)
        r_rev, n_rev = s.rank_batch(users[rev], _excl_pair(held[rev]), exclude_seen=True, exclude=_excl_pair(extra[rev]),
                                    include=_excl_pair(lists[rev]))
        assert np.array_equal(n_rev, n_adm[rev])
        for a, b in zip(_split(r_rev, held[rev]), per[rev]):
            assert np.array_equal(a, b)
        for i in range(len(users)):
            r1, n1 = s.rank_batch(users[i:i + 1], _excl_pair(held[i:i + 1]), exclude_seen=True, exclude=_excl_pair(extra[i:i + 1]),
                                  include=_excl_pair(lists[i:i + 1]))
            assert np.array_equal(r1, per[i]) and n1[0] == n_adm[i], i
        # 5600 entries x the whole catalogue: more include indices than one chunk's index area holds
        reps = 5600
        assert reps * DIMB > api.TOPN_INCLUDE_MAX_ROW, "the batch does not exceed one chunk's index area"
        pick = np.arange(reps) % len(users)
        big_users = users[pick]
        big_held = [held[i] for i in pick]
        ip = np.arange(reps + 1, dtype=np.uint64) * np.uint64(DIMB)
        ii = np.tile(np.arange(DIMB, dtype=np.uint64), reps)
        r_big, n_big = s.rank_batch(big_users, _excl_pair(big_held), exclude_seen=True, include=(ip, ii))
        per_big = _split(r_big, big_held)
        full = (np.array([0, DIMB], np.uint64), np.arange(DIMB, dtype=np.uint64))
        edge = api.TOPN_INCLUDE_MAX_ROW // DIMB                         # the first entry that no longer fits the first chunk
        for e in sorted({0, 1, 205, 206, 207, edge - 1, edge, edge + 1, reps - 1}):
            r1, n1 = s.rank_batch(big_users[e:e + 1], _excl_pair(big_held[e:e + 1]), exclude_seen=True, include=full)
            assert np.array_equal(r1, per_big[e]) and n1[0] == n_big[e], e
        assert np.array_equal(n_big[:len(users)], n_big[len(users):2 * len(users)])
    finally:
        s.close()


def test_edge_rows(prec):
    """6. an empty list and a list wholly excluded give N = 0 with every cell marked; eval_ranking leaves such users out of the means"""
    k = 8
    A, B = _factors(DIMA, DIMB, k, prec, 25)
    s = _session(_matrix(), k, prec, A, B)
    try:
        users = np.array([3, 4, 5, 3], np.uint64)
        held = [np.array([7, 9]), np.array([10, 20, 30]), np.array([1, 2]), np.array([], np.int64)]
        lists = [np.array([], np.int64), np.array([10, 20, 30, 40]), np.array([1, 2, 3, 4, 5]), np.array([], np.int64)]
        excl = [np.array([], np.int64), np.array([5, 10, 20, 30, 40, 50]), np.array([3]), np.array([], np.int64)]
        ranks, n_adm = s.rank_batch(users, _excl_pair(held), exclude=_excl_pair(excl), include=_excl_pair(lists))
        assert n_adm.tolist() == [0, 0, 4, 0]
        assert (ranks[:5] == EXCL).all() and (ranks[5:] < 4).all()
        # through eval_ranking: user 4's held-out items and negatives are all excluded, user 3 has no held-out cell that stays
        X_test = sp.csr_matrix((np.ones(7), ([3, 3, 4, 4, 4, 5, 5], [7, 9, 10, 20, 30, 1, 2])), shape=(DIMA, DIMB))
        E = sp.csr_matrix((np.ones(9), ([3, 3, 4, 4, 4, 4, 4, 4, 5], [7, 9, 5, 10, 20, 30, 40, 50, 3])), shape=(DIMA, DIMB))
        neg = sp.csr_matrix((np.ones(4), ([4, 5, 5, 5], [40, 3, 4, 5])), shape=(DIMA, DIMB))
        out = s.eval_ranking(X_test, k=3, exclude_seen=False, exclude=E, include=neg, per_user=True)
        assert out["n_adm"].tolist() == [0, 0, 4] and out["n_users"] == 1
        assert (out["ranks"][:5] == EXCL).all()
        one = metrics.metrics_from_ranks([0, 2], out["ranks"][5:], [4], 3)
        for name in metrics.METRICS:
            assert out[name] == one[name][0]
    finally:
        s.close()


def test_entry_points_agree(prec):
    """7. the host-pointer entry gives the session's answer; PoisMF.eval_ranking(include=negatives) and Session.eval_ranking agree with
    each other and with metrics_from_ranks on the expected ranks, and are unchanged when the lists already hold the positives"""
    users, seen, extra, lists, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 26)
    csr = _csr()
    s = _session(_matrix(), k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        a = s.rank_batch(users, _excl_pair(held), exclude=_excl_pair(extra), include=_excl_pair(lists))
        b = api.rank_batch(A, B, users, _excl_pair(held), exclude=_excl_pair(extra), include=_excl_pair(lists))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert (a[0] != EXCL).any() and (a[0] == EXCL).any()
        # sampled evaluation: 12 held-out cells and 100 sampled negatives per user, some training cells held out too
        rng = np.random.default_rng(6)
        nt = 12 * DIMA
        X_test = sp.csr_matrix((np.ones(nt), (rng.integers(0, DIMA, nt), rng.integers(0, DIMB, nt))), shape=(DIMA, DIMB))
        X_test = sp.csr_matrix(X_test + csr.multiply(sp.random(DIMA, DIMB, 0.05, random_state=1, format="csr") > 0))
        X_test.sum_duplicates(); X_test.sort_indices()
        neg = sp.csr_matrix((np.ones(100 * DIMA), (np.repeat(np.arange(DIMA), 100), rng.integers(0, DIMB, 100 * DIMA))), shape=(DIMA, DIMB))
        neg.sum_duplicates(); neg.sort_indices()
        with_pos = sp.csr_matrix(neg + X_test)
        everyone = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, everyone, DIMB)
        for sel in (None, np.sort(rng.choice(DIMA, 77, replace=False)).astype(np.uint64)):
            x = s.eval_ranking(X_test, k=10, exclude_seen=True, users=sel, include=neg, per_user=True)
            y = m.eval_ranking(X_test, k=10, exclude=csr, users=sel, include=neg, per_user=True)
            z = s.eval_ranking(X_test, k=10, exclude_seen=True, users=sel, include=with_pos, per_user=True)
            who = np.flatnonzero(np.diff(X_test.indptr)) if sel is None else sel.astype(np.int64)
            pair = _excl_pair([with_pos.indices[with_pos.indptr[u]:with_pos.indptr[u + 1]] for u in who])
            w = s.eval_ranking(X_test, k=10, exclude_seen=True, users=who, include=pair, per_user=True)
            t_rows, l_rows, e_rows = _rows_of(X_test, who), _rows_of(with_pos, who), _rows_of(csr, who)
            want = _expect_all(rows[who], l_rows, e_rows, t_rows)
            assert np.array_equal(x["ranks"], want[0]) and np.array_equal(x["n_adm"], want[1])
            assert (x["ranks"] == EXCL).any() and x["n_users"] > 0
            ref = metrics.mean_metrics(metrics.metrics_from_ranks(x["test_indptr"], want[0], want[1], 10))
            for other in (y, z, w):
                assert np.array_equal(x["ranks"], other["ranks"]) and np.array_equal(x["n_adm"], other["n_adm"])
                assert np.array_equal(x["test_indptr"], other["test_indptr"]) and x["n_users"] == other["n_users"]
                for name in metrics.METRICS:
                    assert x[name] == other[name] or (np.isnan(x[name]) and np.isnan(other[name]))
            for name in metrics.METRICS + ("n_users",):
                assert x[name] == ref[name] or (np.isnan(x[name]) and np.isnan(ref[name]))
    finally:
        s.close()


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_errors_with_a_device(flavour, case):
    """rc 2 and nothing written, through the C entry point itself"""
    users, test, incl, excl = BAD[case]
    rc, rank, n_adm = _c_call(flavour, users, test, incl, excl)
    assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour,kmax", [(False, 256), (True, 512), ("r", 256)], ids=["d", "f", "r"])
def test_c_entry_null_list_and_k_with_a_device(flavour, kmax):
    rc, rank, n_adm = _c_call(flavour, [0, 1], OK_T, OK_I, None, null_incl=True)
    assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)
    for k in (0, kmax + 1):
        rc, rank, n_adm = _c_call(flavour, [0, 1], OK_T, OK_I, None, k=k)
        assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_valid_call_with_a_device(flavour):
    """factors of ones: every score is equal, so a rank is the number of admissible candidates with a smaller index"""
    rc, rank, n_adm = _c_call(flavour, [0, 1, 0, 2], ([0, 3, 3, 5, 6], [0, 4, 7, 2, 299, 5]),
                              ([0, 4, 4, 7, 9], [0, 1, 4, 7, 2, 100, 299, 3, 5]), ([0, 2, 2, 3, 3], [0, 1, 4]))
    assert rc == 0
    assert rank.tolist() == [EXCL, 0, 1, 0, 2, 1]
    assert n_adm.tolist() == [2, 0, 3, 2]
