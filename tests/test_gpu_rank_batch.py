"""Batched exact ranks (include/poismf_hip.h section 1g) on the GPU: ranks against the existing predict path, agreement with the
batched top-N, ties, independence of the batch a user is in (a batch cut by the scratch budget included), the entry points against
each other, one call over 10^5 users, and the argument checks on a machine that has a device.

The expectation of the exact tests is built from Session.predict -- the pair_dot_kernel path: the user's whole score row, minus
E(u), ordered by (score descending, item ascending) with np.lexsort; a held-out item's rank is its position in that list.  Every
comparison of ranks is np.array_equal on integers, and no sampled user or cell is left out."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, harness, metrics, synth
from tests import helpers as H
from tests.test_gpu_topn_batch import DIMA, DIMB, KS, LONG_ROWS, _excl_pair, _factors, _matrix, _rows_of, _sample_users, _score_rows, _session
from tests.test_rank_batch_cpu import BAD, NO_ROW_COUNT, _c_call

pytestmark = pytest.mark.gpu

G = 32                      # thresholds per row of rank_tile_kernel (RB_G): the list lengths around it are cases of their own
EXCL = api.RANK_EXCLUDED


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def _csr():
    csr = sp.csr_matrix(_matrix())
    csr.sum_duplicates(); csr.sort_indices()
    return csr


def _expect(score_row, excluded, held_out):
    """(ranks of held_out, EXCL where excluded; N): positions in the lexsort of the admissible items"""
    idx = np.setdiff1d(np.arange(len(score_row)), np.asarray(excluded, np.int64))
    sc = score_row[idx]
    o = np.lexsort((idx, -sc.astype(np.float64)))          # (the cast is exact; it only keeps -sc in one dtype)
    place = np.full(len(score_row), EXCL, np.int64)
    place[idx[o]] = np.arange(len(idx))
    return place[np.asarray(held_out, np.int64)].astype(np.uint32), len(idx)


def _held_out(rng, users, seen, extra):
    """T(u) per user: list lengths 0, 1, G, G + 1 and several thousand among random short ones; some of the user's seen items and
    some of its extra exclusions are held out too (excluded or not, depending on the case)"""
    sizes = [0, 1, G, G + 1, 5000, 2 * G, 3]
    rows = []
    for i in range(len(users)):
        n = sizes[i] if i < len(sizes) else int(rng.integers(2, 20))
        t = rng.choice(DIMB, n, replace=False)
        if i >= len(sizes) and i % 2 == 0:
            t = np.concatenate((t, seen[i][:3], extra[i][:2]))
        rows.append(np.unique(t).astype(np.int64))
    return rows


def _assert_ranks(got, users, rows, held, excl, what):
    ranks, n_adm = got
    assert ranks.dtype == np.uint32 and n_adm.dtype == np.uint32 and len(n_adm) == len(users)
    assert len(ranks) == sum(len(t) for t in held)
    at = 0
    for i in range(len(users)):
        want, N = _expect(rows[i], excl[i], held[i])
        mine = ranks[at:at + len(held[i])]
        at += len(held[i])
        ok = np.array_equal(mine, want)
        print(f"{what} user {users[i]} cells {len(held[i])} excluded {int((want == EXCL).sum())}: equal ranks {ok} N {int(n_adm[i])} / {N}")
        assert ok, (what, int(users[i]), mine[:20], want[:20])
        assert int(n_adm[i]) == N, (what, int(users[i]), int(n_adm[i]), N)


def _cases(rng, users, csr):
    """the four exclusion cases of a batch: name -> (exclude_seen, list or None, E(u) per user)"""
    seen = _rows_of(csr, users)
    extra = [np.union1d(rng.choice(DIMB, int(rng.integers(0, 300)), replace=False), s[:5]) for s in seen]   # (overlaps the seen row)
    none = [np.empty(0, np.int64)] * len(users)
    both = [np.union1d(a, b) for a, b in zip(seen, extra)]
    return seen, extra, {"plain": (False, None, none), "seen": (True, None, seen), "list": (False, _excl_pair(extra), extra),
                         "both": (True, _excl_pair(extra), both)}


def _batch(rng):
    """61 users, the two long rows among them, plus a repeat of the first: 62, not a multiple of 64"""
    users = _sample_users(rng, 61)
    return np.concatenate((users, users[:1]))


BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_exact_ranks_against_the_predict_path(prec, k):
    """5. out_rank equals each held-out item's position in the lexsort of Session.predict's score row minus E(u); out_n_adm its length"""
    csr = _csr()
    A, B = _factors(DIMA, DIMB, k, prec, 10 + k)
    s = _session(_matrix(), k, prec, A, B)
    try:
        rng = np.random.default_rng(100 + k)
        users = _batch(rng)
        assert len(users) % 64 != 0 and set(LONG_ROWS) <= set(users.tolist())
        rows = _score_rows(s, users, DIMB)
        seen, extra, cases = _cases(rng, users, csr)
        held = _held_out(rng, users, seen, extra)
        assert sorted({len(t) for t in held} & {0, 1, G, G + 1}) == [0, 1, G, G + 1] and max(len(t) for t in held) >= 5000
        for what, (exclude_seen, lst, excl) in cases.items():
            got = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst)
            _assert_ranks(got, users, rows, held, excl, what)
            if what != "plain":
                assert (got[0] == EXCL).any()      # (the sentinel is exercised)
    finally:
        s.close()


def test_agreement_with_topn_batch(prec):
    """6. every cell with rank below 128 sits at topn_batch(users, 128)[u][rank], and every held-out item that topn_batch lists has
    that index as its rank"""
    k = 50
    csr = _csr()
    A, B = _factors(DIMA, DIMB, k, prec, 21)
    B[:400] *= 1.6                                   # (the first 400 items are the best of every user: held-out items among them)
    s = _session(_matrix(), k, prec, A, B)
    try:
        rng = np.random.default_rng(4)
        users = _batch(rng)
        seen, extra, cases = _cases(rng, users, csr)
        held = [np.union1d(t, rng.choice(400, 40, replace=False)) for t in _held_out(rng, users, seen, extra)]
        listed = 0
        for what, (exclude_seen, lst, excl) in cases.items():
            ranks, _ = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst)
            top, _ = s.topn_batch(users, 128, exclude_seen=exclude_seen, exclude=lst)
            at = 0
            for i in range(len(users)):
                r = ranks[at:at + len(held[i])].astype(np.int64)
                at += len(held[i])
                low = r < 128
                assert np.array_equal(top[i][r[low]].astype(np.int64), held[i][low]), (what, int(users[i]))
                where = {int(j): pos for pos, j in enumerate(top[i])}
                for t, rt in zip(held[i], r):
                    if int(t) in where:
                        listed += 1
                        assert where[int(t)] == rt, (what, int(users[i]), int(t), where[int(t)], rt)
        assert listed > 1000                           # (the comparison is not vacuous)
    finally:
        s.close()


@pytest.mark.parametrize("k", [5, 50])
def test_ties(prec, k):
    """7. factors of ones: every score is equal, so rank(u, t) = the number of admissible items with an index below t"""
    csr = _csr()
    s = _session(_matrix(), k, prec, np.ones((DIMA, k), H.dtype_of(prec)), np.ones((DIMB, k), H.dtype_of(prec)))
    try:
        rng = np.random.default_rng(k)
        users = _batch(rng)
        seen, extra, cases = _cases(rng, users, csr)
        held = _held_out(rng, users, seen, extra)
        for what, (exclude_seen, lst, excl) in cases.items():
            ranks, n_adm = s.rank_batch(users, _excl_pair(held), exclude_seen=exclude_seen, exclude=lst)
            at = 0
            for i in range(len(users)):
                e = np.asarray(excl[i], np.int64)
                want = (held[i] - np.searchsorted(e, held[i])).astype(np.uint32)
                want[np.isin(held[i], e)] = EXCL
                assert np.array_equal(ranks[at:at + len(held[i])], want), (what, int(users[i]))
                assert int(n_adm[i]) == DIMB - len(e)
                at += len(held[i])
    finally:
        s.close()


def _rows_of_result(ranks, held):
    out, at = [], 0
    for t in held:
        out.append(ranks[at:at + len(t)])
        at += len(t)
    return out


def test_independence_of_company(prec):
    """8. a user's ranks alone, in a batch of 64, in a batch of 1000 in another order, and in a batch so large that the scratch budget
    cuts it into chunks: identical"""
    k = 50
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    s = _session(_matrix(), k, prec, A, B)
    try:
        rng = np.random.default_rng(8)
        everyone = np.arange(DIMA, dtype=np.uint64)
        held = [np.sort(rng.choice(DIMB, int(rng.integers(0, 24)), replace=False)) for _ in everyone]
        for u in (5, 1777):
            held[u] = np.sort(rng.choice(DIMB, 3000, replace=False))
        r_all, n_all = s.rank_batch(everyone, _excl_pair(held), exclude_seen=True)
        per_all = _rows_of_result(r_all, held)
        order = rng.permutation(DIMA)[:1000]
        r_k, n_k = s.rank_batch(order.astype(np.uint64), _excl_pair([held[u] for u in order]), exclude_seen=True)
        for got, u in zip(_rows_of_result(r_k, [held[u] for u in order]), order):
            assert np.array_equal(got, per_all[u]), int(u)
        assert np.array_equal(n_k, n_all[order])
        for u in (0, 5, 63, 64, 1777, 2999):
            r1, n1 = s.rank_batch([u], _excl_pair([held[u]]), exclude_seen=True)
            assert np.array_equal(r1, per_all[u]) and n1[0] == n_all[u]
            batch = np.concatenate(([u], rng.choice(DIMA, 62, replace=False), [u]))
            r64, n64 = s.rank_batch(batch.astype(np.uint64), _excl_pair([held[v] for v in batch]), exclude_seen=True)
            rows = _rows_of_result(r64, [held[v] for v in batch])
            assert len(batch) == 64 and np.array_equal(rows[0], per_all[u]) and np.array_equal(rows[-1], per_all[u])
            assert n64[0] == n_all[u] and n64[-1] == n_all[u]
        # 3000 users x 1300 held-out cells: more cells than one chunk of the scratch may carry
        big = [np.sort(rng.choice(DIMB, 1300, replace=False)) for _ in everyone]
        n_cells = sum(len(t) for t in big)
        per_cell = 8 * 4 + 2 * A.itemsize
        assert n_cells * per_cell > (api.RANK_BATCH_BUDGET_MB << 20) // 2, "the batch does not exceed what one chunk holds"
        r_big = _rows_of_result(s.rank_batch(everyone, _excl_pair(big), exclude_seen=True)[0], big)
        for u in (0, 5, 1234, 1777, 2500, 2998, 2999):
            r1, _ = s.rank_batch([u], _excl_pair([big[u]]), exclude_seen=True)
            assert np.array_equal(r1, r_big[u]), int(u)
    finally:
        s.close()


def test_rows_in_the_callers_own_order(prec):
    """a session whose resident rows are stored in reversed order (scanned, not binary-searched): the same ranks"""
    k = 50
    coo = _matrix()
    A, B = _factors(DIMA, DIMB, k, prec, 31)
    rng = np.random.default_rng(2)
    users = _batch(rng)
    csr_sp = _csr()
    seen, extra, cases = _cases(rng, users, csr_sp)
    held = _held_out(rng, users, seen, extra)
    s = _session(coo, k, prec, A, B)
    try:
        want = {w: s.rank_batch(users, _excl_pair(held), exclude_seen=es, exclude=lst) for w, (es, lst, _) in cases.items()}
    finally:
        s.close()
    csr, csc = harness.process_data(coo, prec)
    rev = api.Session(H._reorder_rows(csr, "rev", rng), H._reorder_rows(csc, "rev", rng), DIMA, DIMB, k, prec)
    try:
        rev.set_factors(A, B)
        for w, (es, lst, _) in cases.items():
            r, n = rev.rank_batch(users, _excl_pair(held), exclude_seen=es, exclude=lst)
            assert np.array_equal(r, want[w][0]) and np.array_equal(n, want[w][1]), w
    finally:
        rev.close()


def test_entry_points_agree(prec):
    """9. PoisMF.eval_ranking (host pointers) and Session.eval_ranking: identical ranks and metric values; the means are those of
    metrics_from_ranks on the raw ranks"""
    k = 50
    coo = _matrix()
    csr = _csr()
    A, B = _factors(DIMA, DIMB, k, prec, 41)
    rng = np.random.default_rng(6)
    nt = 12 * DIMA
    X_test = sp.csr_matrix((np.ones(nt), (rng.integers(0, DIMA, nt), rng.integers(0, DIMB, nt))), shape=(DIMA, DIMB))
    X_test = X_test + csr.multiply(sp.random(DIMA, DIMB, 0.02, random_state=1, format="csr") > 0)    # (some training cells are held out too)
    s = _session(coo, k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        for users in (None, _sample_users(rng, 100)):
            a = s.eval_ranking(X_test, k=10, exclude_seen=True, users=users, per_user=True)
            b = m.eval_ranking(X_test, k=10, exclude=csr, users=users, per_user=True)
            c = s.eval_ranking(X_test, k=10, exclude_seen=False, exclude=csr, users=users, per_user=True)
            assert (a["ranks"] == EXCL).any() and a["n_users"] > 0
            for other in (b, c):
                assert np.array_equal(a["ranks"], other["ranks"]) and np.array_equal(a["n_adm"], other["n_adm"])
                assert np.array_equal(a["test_indptr"], other["test_indptr"]) and a["n_users"] == other["n_users"]
                for name in metrics.METRICS:
                    assert a[name] == other[name] or (np.isnan(a[name]) and np.isnan(other[name]))
                    assert np.array_equal(a["per_user"][name], other["per_user"][name], equal_nan=True)
            raw = metrics.metrics_from_ranks(a["test_indptr"], a["ranks"], a["n_adm"], 10)
            means = metrics.mean_metrics(raw)
            short = s.eval_ranking(X_test, k=10, exclude_seen=True, users=users)
            assert set(short) == set(metrics.METRICS) | {"n_users"}
            for name in metrics.METRICS + ("n_users",):
                assert means[name] == a[name] == short[name]
        # the raw calls agree as well, and with the model-level wrapper on all of A
        everyone = np.arange(DIMA)
        test_rows = sp.csr_matrix(X_test)
        test_rows.sum_duplicates(); test_rows.sort_indices()
        r1 = s.rank_batch(everyone, test_rows)
        r2 = api.rank_batch(A, B, everyone, test_rows)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and np.all(r1[1] == DIMB)
    finally:
        s.close()


def test_size_many_users_in_one_call():
    """10. 10^5 users x 25000 items, about ten held-out cells each, k = 50, fp32, seen items excluded: one call, and 256 sampled
    users against the predict path"""
    n_users, n_items, k = 10 ** 5, 25000, 50
    t = synth.uniform_triplets(n_users, n_items, 4 * 10 ** 6, seed=5)
    A, B = _factors(n_users, n_items, k, True, 8)
    rng = np.random.default_rng(1)
    nt = 10 * n_users
    X_test = sp.csr_matrix((np.ones(nt), (rng.integers(0, n_users, nt), rng.integers(0, n_items, nt))), shape=(n_users, n_items))
    X_test.sum_duplicates(); X_test.sort_indices()
    s = api.Session.from_coo(t, k, True)
    try:
        s.set_factors(A, B)
        users = np.arange(n_users, dtype=np.uint64)
        ranks, n_adm = s.rank_batch(users, X_test, exclude_seen=True)
        assert len(ranks) == X_test.nnz
        X = sp.csr_matrix((np.ones(len(t.row), np.float32), (t.row, t.col)), shape=t.shape)
        X.sum_duplicates(); X.sort_indices()
        assert np.array_equal(n_adm, (n_items - np.diff(X.indptr)).astype(np.uint32))
        sample = np.sort(rng.choice(n_users, 256, replace=False))
        rows = _score_rows(s, sample, n_items)
        held = _rows_of(X_test, sample)
        got = np.concatenate([ranks[X_test.indptr[u]:X_test.indptr[u + 1]] for u in sample])
        _assert_ranks((got, n_adm[sample]), sample, rows, held, _rows_of(X, sample), "size")
        out = s.eval_ranking(X_test, k=10)
        assert out["n_users"] > 0.99 * n_users and 0.45 < out["auc"] < 0.55      # (random factors: no better than chance)
    finally:
        s.close()


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_errors_with_a_device(flavour, case):
    """rc 2 and nothing written, through the C entry point itself"""
    users, test, excl = BAD[case]
    rc, rank, n_adm = _c_call(flavour, users, test, excl)
    assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_valid_call_with_a_device(flavour):
    rc, rank, n_adm = _c_call(flavour, [0, 1, 0, 2], ([0, 3, 3, 5, 6], [0, 4, 7, 2, 299, 5]), ([0, 2, 2, 3, 3], [0, 1, 4]))
    assert rc == 0
    # all scores are equal (factors of ones): a rank is the number of admissible items below the item
    assert rank.tolist() == [EXCL, 2, 5, 2, 298, 5]
    assert n_adm.tolist() == [298, 300, 299, 300]


def test_exclude_seen_outside_the_shard(prec):
    """exclude_seen on a session created with a partial shardA, for a user outside it: rc 2 from the library itself"""
    k = 8
    coo = _matrix()
    csr, csc = harness.process_data(coo, prec)
    A, B = _factors(DIMA, DIMB, k, prec, 3)
    s = api.Session(csr, csc, DIMA, DIMB, k, prec, shardA=(1000, 2000), shardB=(0, DIMB))
    try:
        s.set_factors(A, B)
        users = np.array([1500, 2000], np.uint64)
        tp, ti = np.array([0, 1, 2], np.uint64), np.array([7, 9], np.uint64)
        rank, n_adm = np.full(2, 12345, np.uint32), np.full(2, 54321, np.uint32)
        p = api._ptr
        rc = s.lib.poismf_hip_session_rank_batch(s.h, p(users), 2, p(tp), p(ti), 1, None, None, p(rank), p(n_adm))
        assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)
        with pytest.raises(ValueError):
            s.rank_batch(users, (tp, ti), exclude_seen=True)
        inside = np.array([1000, 1500, 1999], np.uint64)
        held = [np.array([3, 500, 24999]), np.array([], np.int64), np.array([0])]
        sp_csr = _csr()
        rows = _score_rows(s, inside, DIMB)
        _assert_ranks(s.rank_batch(inside, _excl_pair(held), exclude_seen=True), inside, rows, held, _rows_of(sp_csr, inside), "shard")
        r, n = s.rank_batch(users, (tp, ti))       # without exclude_seen any user of A may be asked for
        assert np.all(n == DIMB) and np.all(r < DIMB)
    finally:
        s.close()


def test_fitted_model_end_to_end():
    """C1: fit, hold the training cells out against themselves (all excluded), then a real split: metrics in range"""
    coo = synth.readme_coo()
    csr = sp.csr_matrix(coo)
    csr.sum_duplicates(); csr.sort_indices()
    rng = np.random.default_rng(0)
    mask = rng.random(csr.nnz) < 0.2
    c = csr.tocoo()
    train = sp.csr_matrix((c.data[~mask], (c.row[~mask], c.col[~mask])), shape=csr.shape)
    test = sp.csr_matrix((c.data[mask], (c.row[mask], c.col[mask])), shape=csr.shape)
    m = api.PoisMF(k=5, method="cg").fit(train.tocoo())
    out = m.eval_ranking(test, k=10, exclude=train, per_user=True)
    assert out["n_users"] == int((np.diff(test.indptr) > 0).sum()) and not (out["ranks"] == EXCL).any()
    for name in metrics.METRICS:
        assert 0.0 <= out[name] <= 1.0
    scores = m.A.astype(np.float64) @ m.B.astype(np.float64).T
    u = int(np.flatnonzero(np.diff(test.indptr))[0])
    held = test.indices[test.indptr[u]:test.indptr[u + 1]]
    got = out["ranks"][:len(held)]
    seen = train.indices[train.indptr[u]:train.indptr[u + 1]]
    adm = np.setdiff1d(np.arange(csr.shape[1]), seen)
    for t, r in zip(held, got):        # float64 truth: the items that beat t by more than rounding are before it, and no others far behind
        assert int((scores[u, adm] > scores[u, t] * (1 + 1e-4)).sum()) <= int(r) <= int((scores[u, adm] >= scores[u, t] * (1 - 1e-4)).sum())
    gone = m.eval_ranking(train, k=10, exclude=train)
    assert gone["n_users"] == 0 and np.isnan(gone["auc"])
