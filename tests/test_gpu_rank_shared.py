"""Batched exact ranks among candidate lists shared between users (include/poismf_hip.h section 1k) on the GPU: ranks and admissible
counts against the existing predict path in both modes, identity with section 1j given every user's list written out (united with
its held-out row in the united mode), with the dense call of section 1g given the complement and with the batched top-N of section
1i over the same table, ties and the phantom rows past a list's end, independence of the company a user is in (slices and chunks
included), empty and wholly excluded lists, the entry points against each other, and the C entry on a machine that has a device.

The expectation is built from Session.predict -- the pair_dot_kernel path: the user's whole score row restricted to C(u), ordered by
(score descending, item ascending) with np.lexsort; a held-out item's rank is its position in that list.  Every comparison of ranks
is np.array_equal on integers, and no user or cell is left out.

Shapes: 300 users x 3077 items; a table of lists of 0, 1, 63, 64, 65, 129, 1000 and 3077 items plus one nobody refers to; 1, 63, 64,
65 and 130 batch entries on one list, so that tile boundaries fall inside and between lists (with 323 entries on those five alone,
users repeat); held-out rows of 0, 1, 32, 33 and 65 cells (the group size and across it) among random short ones."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, metrics
from tests.test_gpu_rank_include import _assert_ranks, _cases, _csr, _expect_all, _matrix, _split
from tests.test_gpu_topn_batch import KS, _excl_pair, _factors, _rows_of, _score_rows, _session
from tests.test_rank_shared_cpu import BAD, NO_ROW_COUNT, OK_L, OK_OF, OK_T, _c_call, _untouched

pytestmark = pytest.mark.gpu

DIMA, DIMB = 300, 3077
EXCL = api.RANK_EXCLUDED
LENGTHS = [0, 1, 63, 64, 65, 129, 1000, DIMB, 500]          # the table; nobody refers to the last list
ENTRIES = [2, 1, 63, 64, 65, 130, 7, 4, 0]                   # batch entries per list
SPECIAL = {5: [0, 1, 32, 33, 65], 7: [65, 33]}               # list -> held-out cells of its first entries, all drawn from the list
ZERO_USER = 17                                               # its row of A is zeroed; it sits on the lists of 129 and of 1000


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


@functools.lru_cache(maxsize=None)
def _plan(seed=0):
    """The batch, built once and never changed: the table, users (336 entries in a shuffled order of lists), list_of, their seen
    rows, extra exclusions and held-out rows -- cells from the list, from outside it, from the user's seen row and from its extra
    exclusions."""
    rng = np.random.default_rng(seed)
    table = [np.sort(rng.choice(DIMB, n, replace=False)).astype(np.int64) for n in LENGTHS]
    of = rng.permutation(np.repeat(np.arange(len(LENGTHS)), ENTRIES))
    m = len(of)
    users = np.concatenate((rng.permutation(DIMA), rng.integers(0, DIMA, m - DIMA)))
    users[users == ZERO_USER] = ZERO_USER + 1
    users[np.flatnonzero(of == 5)[7]] = ZERO_USER                                       # 129 = 2 x 64 + 1: 63 phantom rows in its last step
    users[np.flatnonzero(of == 6)[2]] = ZERO_USER
    seen = _rows_of(_csr(), users)
    extra = [np.union1d(rng.choice(DIMB, int(rng.integers(0, 40)), replace=False), s[:3]) for s in seen]   # (overlaps the seen row)
    # some seen and excluded items are listed: the lists of 1000 and of everything hold many by chance, the others are given a few
    held, nth = [], {}
    for i in range(m):
        g = int(of[i])
        lst = table[g]
        nth[g] = nth.get(g, -1) + 1
        if g in SPECIAL and nth[g] < len(SPECIAL[g]):
            t = rng.choice(lst, SPECIAL[g][nth[g]], replace=False)
        else:
            own = rng.choice(lst, min(len(lst), int(rng.integers(0, 8))), replace=False) if len(lst) else np.empty(0, np.int64)
            listed_excl = np.intersect1d(lst, np.union1d(seen[i], extra[i]))[:2]
            t = np.concatenate((own, rng.choice(DIMB, int(rng.integers(0, 4)), replace=False), seen[i][:2], extra[i][:2], listed_excl))
        held.append(np.unique(t).astype(np.int64))
    assert m == sum(ENTRIES) == 336 and m % 64 != 0 and len(np.unique(users)) < m
    assert {0, 1, 32, 33, 65} <= {len(t) for t in held}
    assert (users == ZERO_USER).sum() == 2 and all(len(held[i]) for i in np.flatnonzero(users == ZERO_USER))
    return users.astype(np.uint64), of.astype(np.uint64), table, seen, extra, held


def _lists(table, of, held, unite):
    """C(u) before exclusion, per batch entry"""
    return [np.union1d(table[int(g)], t) if unite else table[int(g)] for g, t in zip(of, held)]


def _zeroed(A):
    A = A.copy()
    A[ZERO_USER] = 0
    return A


def _call(s, users, held, table, of, unite, exclude_seen=False, exclude=None):
    return s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=exclude, include=_excl_pair(table), include_of=of,
                        unite_test=unite)


BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_exact_ranks_against_the_predict_path(prec, k):
    """1. out_rank equals each held-out item's position in the lexsort of Session.predict's scores over C(u), in both modes and the
    four exclusion cases; out_n_adm its length.  The user whose row of A is zero ranks by item index alone, also on a list whose
    length is no multiple of 64: a phantom row past the list's end must not be counted."""
    users, of, table, seen, extra, held = _plan()
    A, B = _factors(DIMA, DIMB, k, prec, 10 + k)
    s = _session(_matrix(), k, prec, _zeroed(A), B)
    try:
        rows = _score_rows(s, users, DIMB)
        assert not rows[users == ZERO_USER].any()
        for unite in (False, True):
            lists = _lists(table, of, held, unite)
            for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
                got = _call(s, users, held, table, of, unite, exclude_seen, lst)
                _assert_ranks(got, _expect_all(rows, lists, excl, held), held, f"{what} unite={unite}")
                per = _split(got[0], held)
                for i in np.flatnonzero(users == ZERO_USER):      # the count of admissible smaller indices, written out
                    adm = np.setdiff1d(lists[i], excl[i])
                    want = [int((adm < t).sum()) if t in adm else EXCL for t in held[i]]
                    assert per[i].tolist() == want and got[1][i] == len(adm), (what, unite, i)
                unlisted = [~np.isin(t, table[int(g)]) & ~np.isin(t, e) for t, g, e in zip(held, of, excl)]
                assert sum(int(u.sum()) for u in unlisted) > 100
                for r, u in zip(per, unlisted):                   # an unlisted cell is marked exactly when the mode is not united
                    assert ((r[u] == EXCL) != unite).all()
                if what != "plain":
                    assert any((r[np.isin(t, e)] == EXCL).all() and (np.isin(t, e) & np.isin(t, table[int(g)])).any()
                               for r, t, g, e in zip(per, held, of, excl))
    finally:
        s.close()


def test_identity_with_rank_include_and_the_dense_call(prec):
    """2. and 3. section 1j with every user's list written out (united with its held-out row by _unite_rows in the united mode), and
    section 1g with E(u) united with the complement of C(u): identical ranks and N"""
    users, of, table, seen, extra, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 21)
    s = _session(_matrix(), k, prec, _zeroed(A), B)
    try:
        everything = np.arange(DIMB)
        written = _excl_pair([table[int(g)] for g in of])
        for unite in (False, True):
            incl = api._unite_rows(written, _excl_pair(held)) if unite else written
            lists = _lists(table, of, held, unite)
            for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
                got = _call(s, users, held, table, of, unite, exclude_seen, lst)
                per_user = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst, include=incl)
                assert np.array_equal(got[0], per_user[0]) and np.array_equal(got[1], per_user[1]), (what, unite)
                e_rows = extra if lst is not None else [np.empty(0, np.int64)] * len(users)
                dense_excl = [np.union1d(e, np.setdiff1d(everything, l)) for e, l in zip(e_rows, lists)]
                dense = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=_excl_pair(dense_excl))
                assert np.array_equal(got[0], dense[0]) and np.array_equal(got[1], dense[1]), (what, unite)
                assert (got[0] != EXCL).sum() > 500
    finally:
        s.close()


def test_agreement_with_topn_shared(prec):
    """4. every listed cell with rank below 128 sits at topn_batch(include=table, include_of=, top_n=128)[u][rank], and a padded tail
    is 128 - N long"""
    users, of, table, seen, extra, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 22)
    s = _session(_matrix(), k, prec, _zeroed(A), B)
    try:
        listed = 0
        for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
            ranks, n_adm = _call(s, users, held, table, of, False, exclude_seen, lst)
            top, _ = s.topn_batch(users, 128, exclude_seen=exclude_seen, exclude=lst, include=_excl_pair(table), include_of=of)
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
    """5. 37 distinct rows of B repeated down the catalogue and two zero columns: many equal scores; ranks still equal the lexsort,
    and every unmarked rank is below N (a held-out item never comes before itself)"""
    users, of, table, seen, extra, held = _plan()
    A, B = _factors(DIMA, DIMB, k, prec, 23)
    B = np.ascontiguousarray(B[np.arange(DIMB) % 37])
    B[:, :2] = 0
    s = _session(_matrix(), k, prec, _zeroed(A), B)
    try:
        rows = _score_rows(s, users, DIMB)
        assert len(np.unique(rows[0])) <= 37
        for unite in (False, True):
            lists = _lists(table, of, held, unite)
            for what, (exclude_seen, lst, excl) in _cases(seen, extra).items():
                got = _call(s, users, held, table, of, unite, exclude_seen, lst)
                _assert_ranks(got, _expect_all(rows, lists, excl, held), held, f"{what} unite={unite}")
                for r, n in zip(_split(got[0], held), got[1]):
                    assert (r[r != EXCL] < n).all()
    finally:
        s.close()


def test_independence_of_company(prec):
    """6. a batch entry's ranks alone (one tile on its list: the planner slices every list of more than 64 items), in the batch (whose
    sorted entries fill tiles: few slices or none), in the reversed batch and with the table's rows permuted are identical; so are
    those of a batch that the layout cuts into two chunks, on both sides of the cut"""
    users, of, table, seen, extra, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 24)
    s = _session(_matrix(), k, prec, _zeroed(A), B)
    try:
        for unite in (False, True):
            kw = dict(exclude_seen=True)
            ranks, n_adm = _call(s, users, held, table, of, unite, exclude=_excl_pair(extra), **kw)
            per = _split(ranks, held)
            rev = slice(None, None, -1)
            r_rev, n_rev = _call(s, users[rev], held[rev], table, of[rev], unite, exclude=_excl_pair(extra[rev]), **kw)
            assert np.array_equal(n_rev, n_adm[rev]) and np.array_equal(r_rev, np.concatenate(per[rev]))
            perm = np.random.default_rng(5).permutation(len(table))          # row perm[g] of the new table is the old row g
            new_table = [None] * len(table)
            for g, at in enumerate(perm):
                new_table[at] = table[g]
            r_perm, n_perm = _call(s, users, held, new_table, perm[of.astype(np.int64)].astype(np.uint64), unite, exclude=_excl_pair(extra), **kw)
            assert np.array_equal(r_perm, ranks) and np.array_equal(n_perm, n_adm)
            for i in range(len(users)):
                r1, n1 = _call(s, users[i:i + 1], held[i:i + 1], table, of[i:i + 1], unite, exclude=_excl_pair(extra[i:i + 1]), **kw)
                assert np.array_equal(r1, per[i]) and n1[0] == n_adm[i], (unite, i)
            # the planner slices this one too: 12 entries with a whole-catalogue held-out row on the list of everything are 1164 groups in
            # 19 tiles, far below the workgroups it aims at, over 49 steps
            pick = np.arange(12) * 7
            everything = [np.arange(DIMB)] * len(pick)
            r_long, n_long = _call(s, users[pick], everything, table, 7, unite, **kw)
            for e, i in enumerate(pick):
                r1, n1 = _call(s, users[i:i + 1], everything[:1], table, 7, unite, **kw)
                assert np.array_equal(r1, _split(r_long, everything)[e]) and n1[0] == n_long[e], (unite, i)
        # chunks: the cheapest trigger the layout offers is a chunk's held-out cells; 172 entries with whole-catalogue held-out rows
        reps = 172
        assert reps * DIMB > api.RANK_SHARED_CHUNK_CELLS > (reps - 2) * DIMB, "the batch does not exceed one chunk's held-out cells"
        pick = np.arange(reps) % len(users)
        big_users, big_of = users[pick], of[pick]
        big_held = [np.arange(DIMB)] * reps
        r_big, n_big = _call(s, big_users, big_held, table, big_of, True, exclude_seen=True)
        per_big = _split(r_big, big_held)
        edge = api.RANK_SHARED_CHUNK_CELLS // DIMB                          # the first entry that no longer fits the first chunk
        assert 1 < edge < reps - 1
        for e in sorted({0, 1, edge - 1, edge, edge + 1, reps - 1}):
            r1, n1 = _call(s, big_users[e:e + 1], big_held[e:e + 1], table, big_of[e:e + 1], True, exclude_seen=True)
            assert np.array_equal(r1, per_big[e]) and n1[0] == n_big[e], e
    finally:
        s.close()


def test_edge_rows(prec):
    """7. an empty list and a list wholly excluded give N = 0 with every cell marked -- plus the united positives in the united mode;
    eval_ranking leaves users without a counting cell out of the means"""
    k = 8
    A, B = _factors(DIMA, DIMB, k, prec, 25)
    s = _session(_matrix(), k, prec, A, B)
    try:
        users = np.array([3, 4, 5, 3], np.uint64)
        held = [np.array([7, 9]), np.array([10, 20, 30]), np.array([1, 2]), np.array([], np.int64)]
        table = [np.array([], np.int64), np.array([10, 20, 30, 40]), np.array([1, 2, 3, 4, 5])]
        of = np.array([0, 1, 2, 0], np.uint64)
        excl = [np.array([], np.int64), np.array([5, 10, 20, 30, 40, 50]), np.array([3]), np.array([], np.int64)]
        ranks, n_adm = _call(s, users, held, table, of, False, exclude=_excl_pair(excl))
        assert n_adm.tolist() == [0, 0, 4, 0]
        assert (ranks[:5] == EXCL).all() and (ranks[5:] < 4).all()
        ranks, n_adm = _call(s, users, held, table, of, True, exclude=_excl_pair(excl))
        assert n_adm.tolist() == [2, 0, 4, 0]
        assert sorted(ranks[:2].tolist()) == [0, 1] and (ranks[2:5] == EXCL).all() and (ranks[5:] < 4).all()
        # through eval_ranking: user 4's held-out items and pool are all excluded, user 3 is on the empty pool with its positives excluded
        X_test = sp.csr_matrix((np.ones(7), ([3, 3, 4, 4, 4, 5, 5], [7, 9, 10, 20, 30, 1, 2])), shape=(DIMA, DIMB))
        E = sp.csr_matrix((np.ones(9), ([3, 3, 4, 4, 4, 4, 4, 4, 5], [7, 9, 5, 10, 20, 30, 40, 50, 3])), shape=(DIMA, DIMB))
        pools = sp.csr_matrix((np.ones(4), ([1, 2, 2, 2], [40, 3, 4, 5])), shape=(3, DIMB))
        pool_of = np.zeros(DIMA, np.int64)
        pool_of[4], pool_of[5] = 1, 2
        out = s.eval_ranking(X_test, k=3, exclude_seen=False, exclude=E, include=pools, include_of=pool_of, per_user=True)
        assert out["n_adm"].tolist() == [0, 0, 4] and out["n_users"] == 1
        assert (out["ranks"][:5] == EXCL).all()
        one = metrics.metrics_from_ranks([0, 2], out["ranks"][5:], [4], 3)
        for name in metrics.METRICS:
            assert out[name] == one[name][0]
    finally:
        s.close()


def test_entry_points_agree(prec):
    """8. the host-pointer entry gives the session's answer; PoisMF.eval_ranking(include=pools, include_of=) and Session.eval_ranking
    agree with each other, with eval_ranking(include=<the pools written out per user>) and with metrics_from_ranks on the expected
    ranks, for users=None and for a subset"""
    users, of, table, seen, extra, held = _plan()
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 26)
    csr = _csr()
    s = _session(_matrix(), k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        for unite in (False, True):
            a = _call(s, users, held, table, of, unite, exclude=_excl_pair(extra))
            b = api.rank_batch(A, B, users, _excl_pair(held), exclude=_excl_pair(extra), include=_excl_pair(table), include_of=of, unite_test=unite)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert (a[0] != EXCL).any() and (a[0] == EXCL).any()
        # sampled evaluation: 12 held-out cells per user, some training cells held out too; three pools of 100, 1000 and no negatives
        rng = np.random.default_rng(6)
        nt = 12 * DIMA
        X_test = sp.csr_matrix((np.ones(nt), (rng.integers(0, DIMA, nt), rng.integers(0, DIMB, nt))), shape=(DIMA, DIMB))
        X_test = sp.csr_matrix(X_test + csr.multiply(sp.random(DIMA, DIMB, 0.05, random_state=1, format="csr") > 0))
        X_test.sum_duplicates(); X_test.sort_indices()
        pool_rows = [np.sort(rng.choice(DIMB, n, replace=False)) for n in (100, 1000, 0)]
        pools = sp.csr_matrix((np.ones(1100), (np.repeat([0, 1], [100, 1000]), np.concatenate(pool_rows))), shape=(3, DIMB))
        pool_of = rng.integers(0, 3, DIMA)
        written = sp.csr_matrix((np.ones(sum(len(pool_rows[g]) for g in pool_of)),
                                 (np.repeat(np.arange(DIMA), [len(pool_rows[g]) for g in pool_of]), np.concatenate([pool_rows[g] for g in pool_of]))),
                                shape=(DIMA, DIMB))
        everyone = np.arange(DIMA, dtype=np.uint64)
        rows = _score_rows(s, everyone, DIMB)
        for sel in (None, np.sort(rng.choice(DIMA, 77, replace=False)).astype(np.uint64)):
            x = s.eval_ranking(X_test, k=10, exclude_seen=True, users=sel, include=pools, include_of=pool_of, per_user=True)
            y = m.eval_ranking(X_test, k=10, exclude=csr, users=sel, include=pools, include_of=pool_of, per_user=True)
            z = s.eval_ranking(X_test, k=10, exclude_seen=True, users=sel, include=written, per_user=True)
            who = np.flatnonzero(np.diff(X_test.indptr)) if sel is None else sel.astype(np.int64)
            t_rows, e_rows = _rows_of(X_test, who), _rows_of(csr, who)
            l_rows = [np.union1d(pool_rows[pool_of[u]], t) for u, t in zip(who, t_rows)]
            want = _expect_all(rows[who], l_rows, e_rows, t_rows)
            assert np.array_equal(x["ranks"], want[0]) and np.array_equal(x["n_adm"], want[1])
            assert (x["ranks"] == EXCL).any() and x["n_users"] > 0
            ref = metrics.mean_metrics(metrics.metrics_from_ranks(x["test_indptr"], want[0], want[1], 10))
            for other in (y, z):
                assert np.array_equal(x["ranks"], other["ranks"]) and np.array_equal(x["n_adm"], other["n_adm"])
                assert np.array_equal(x["test_indptr"], other["test_indptr"]) and x["n_users"] == other["n_users"]
                for name in metrics.METRICS:
                    assert x[name] == other[name] or (np.isnan(x[name]) and np.isnan(other[name]))
            for name in metrics.METRICS + ("n_users",):
                assert x[name] == ref[name] or (np.isnan(x[name]) and np.isnan(ref[name]))
        # one pool for everybody, named by one int
        x = s.eval_ranking(X_test, k=10, exclude_seen=True, include=pools, include_of=1, per_user=True)
        y = s.eval_ranking(X_test, k=10, exclude_seen=True, include=pools, include_of=np.ones(DIMA, np.int64), per_user=True)
        assert np.array_equal(x["ranks"], y["ranks"]) and np.array_equal(x["n_adm"], y["n_adm"])
    finally:
        s.close()


FLAVOURS = pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])


@FLAVOURS
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_errors_with_a_device(flavour, case):
    """9. rc 2 and nothing written, through the C entry point itself"""
    users, test, tbl, list_of, excl = BAD[case]
    for unite in (0, 1):
        assert _untouched(*_c_call(flavour, users, test, tbl, list_of, excl, unite=unite))


@pytest.mark.parametrize("flavour,kmax", [(False, 256), (True, 512), ("r", 256)], ids=["d", "f", "r"])
def test_c_entry_null_pointers_and_k_with_a_device(flavour, kmax):
    for which in ("test_indptr", "list_indptr", "list_of"):
        assert _untouched(*_c_call(flavour, [0, 1], OK_T, OK_L, OK_OF, None, null=(which,)))
    assert _untouched(*_c_call(flavour, [0, 1], OK_T, ([0], []), [0, 0], None, n_lists=0))
    for k in (0, kmax + 1):
        assert _untouched(*_c_call(flavour, [0, 1], OK_T, OK_L, OK_OF, None, k=k))


@FLAVOURS
def test_c_entry_valid_call_with_a_device(flavour):
    """factors of ones: every score is equal, so a rank is the number of admissible candidates with a smaller index.  Lists
    {0, 1, 4, 7}, {} and {2, 100, 299}; four entries on lists 0, 1, 2, 0 with exclusions {0, 1}, {}, {100}, {}."""
    users, of = [0, 1, 0, 2], [0, 1, 2, 0]
    test = ([0, 4, 5, 8, 9], [0, 3, 4, 7, 9, 2, 50, 299, 5])
    tbl = ([0, 4, 4, 7], [0, 1, 4, 7, 2, 100, 299])
    excl = ([0, 2, 2, 3, 3], [0, 1, 100])
    rc, rank, n_adm = _c_call(flavour, users, test, tbl, of, excl, unite=0)
    assert rc == 0
    assert rank.tolist() == [EXCL, EXCL, 0, 1, EXCL, 0, EXCL, 1, EXCL]
    assert n_adm.tolist() == [2, 0, 2, 4]
    rc, rank, n_adm = _c_call(flavour, users, test, tbl, of, excl, unite=1)
    assert rc == 0
    assert rank.tolist() == [EXCL, 0, 1, 2, 0, 0, 1, 2, 3]
    assert n_adm.tolist() == [3, 1, 3, 5]
