"""Batched top-N (include/poismf_hip.h section 1f) on the GPU: bits against the existing predict path, independence of the
batch a user is in, ties, float64 truth, the host-pointer entry and PoisMF.topN_batch, one call over 10^5 users, the argument
checks on a machine that has a device, and lists that are exactly full through the three kernels that share the selection.

The expectation of the exact tests is built from Session.predict -- the pair_dot_kernel path, which the batched code does not
share: the user's whole score row, minus E(u), ordered by (score descending, item ascending) with np.lexsort.  No sampled user
is left out and nothing but tests.helpers.check_topn has a tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bindings
from poismf_amd import api, harness, synth
from tests import helpers as H
from tests.test_topn_batch_cpu import BAD, _c_call

pytestmark = pytest.mark.gpu

DIMA, DIMB = 3000, 25000
LONG_ROWS = {5: 5000, 1777: 6500}   # two rows longer than 4096


def T(is_float, t64, t32):
    return t32 if is_float else t64


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def _matrix(seed=3):
    """uniform 3000 x 25000 with ~40 nonzeros per row, plus the two long rows; SciPy COO with float64 counts"""
    rng = np.random.default_rng(seed)
    nnz = 40 * DIMA
    row = [rng.integers(0, DIMA, nnz)]
    col = [rng.integers(0, DIMB, nnz)]
    for r, n in LONG_ROWS.items():
        row.append(np.full(n, r))
        col.append(rng.choice(DIMB, n, replace=False))
    row, col = np.concatenate(row), np.concatenate(col)
    return sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(DIMA, DIMB))


def _factors(dimA, dimB, k, prec, seed):
    rng = np.random.default_rng(seed)
    dt = H.dtype_of(prec)
    return rng.random((dimA, k)).astype(dt), rng.random((dimB, k)).astype(dt)


def _session(coo, k, prec, A, B):
    s = api.Session.from_coo(coo, k, prec)
    s.set_factors(A, B)
    return s


def _score_rows(s, users, dimB):
    """the users' whole score rows from the existing predict path: [len(users) x dimB]"""
    users = np.asarray(users, np.uint64)
    out = s.predict(np.repeat(users, dimB), np.tile(np.arange(dimB, dtype=np.uint64), len(users)))
    return out.reshape(len(users), dimB)


def _expect(score_row, excluded, n):
    """first n admissible items under (score descending, item ascending), and their scores"""
    idx = np.setdiff1d(np.arange(len(score_row)), np.asarray(excluded, np.int64))
    sc = score_row[idx]
    o = np.lexsort((idx, -sc.astype(np.float64)))[:n]   # (the cast is exact; it only keeps -sc in one dtype)
    return idx[o].astype(np.uint64), sc[o]


def _rows_of(csr, users):
    return [csr.indices[csr.indptr[u]:csr.indptr[u + 1]] for u in users]


def _excl_pair(rows):
    """(indptr, indices) of per-user sorted exclusion lists"""
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if len(rows) else np.empty(0)).astype(np.uint64)


def _sample_users(rng, n):
    u = rng.choice(DIMA, n, replace=False)
    u[:len(LONG_ROWS)] = list(LONG_ROWS)   # the long rows are always among them
    return np.unique(u)


def _assert_rows(got, users, rows, excl, n, what):
    ix, sc = got
    assert ix.shape == (len(users), n) and sc.shape == (len(users), n)
    for i in range(len(users)):
        eix, esc = _expect(rows[i], excl[i], n)
        print(f"{what} user {users[i]} n {n}: equal ix {np.array_equal(ix[i], eix)} equal score {np.array_equal(sc[i], esc)}")
        assert np.array_equal(ix[i], eix), (what, int(users[i]), n, ix[i], eix)
        assert np.array_equal(sc[i], esc), (what, int(users[i]), n)


KS = [1, 3, 4, 5, 50, 64, 65, 100, 200, 256]
BIT_CASES = [(p, k) for p in (False, True) for k in KS] + [(True, 512)]   # (an fp64 session supports k <= 256)


@pytest.mark.parametrize("prec,k", BIT_CASES, ids=[f"{'f32' if p else 'f64'}-k{k}" for p, k in BIT_CASES])
def test_bits_against_the_predict_path(prec, k):
    """1. indices and scores array_equal to the lexsort of Session.predict's score row minus E(u)"""
    coo = _matrix()
    csr = sp.csr_matrix(coo)
    csr.sum_duplicates(); csr.sort_indices()
    A, B = _factors(DIMA, DIMB, k, prec, 10 + k)
    s = _session(coo, k, prec, A, B)
    try:
        rng = np.random.default_rng(k)
        users = _sample_users(rng, 64)
        rows = _score_rows(s, users, DIMB)
        seen = _rows_of(csr, users)
        extra = [np.sort(rng.choice(DIMB, int(rng.integers(0, 300)), replace=False)) for _ in users]
        none = [np.empty(0, np.int64)] * len(users)
        both = [np.union1d(a, b) for a, b in zip(seen, extra)]
        for n in (1, 10, 128):
            _assert_rows(s.topn_batch(users, n, output_score=True), users, rows, none, n, "plain")
            _assert_rows(s.topn_batch(users, n, exclude_seen=True, output_score=True), users, rows, seen, n, "seen")
            _assert_rows(s.topn_batch(users, n, exclude=_excl_pair(extra), output_score=True), users, rows, extra, n, "extra")
            _assert_rows(s.topn_batch(users, n, exclude_seen=True, exclude=_excl_pair(extra), output_score=True), users, rows, both, n, "both")
    finally:
        s.close()


def test_independence_of_company(prec):
    """2. alone, among all users, in a reversed batch, listed three times: identical rows"""
    k = 50
    coo = _matrix()
    A, B = _factors(DIMA, DIMB, k, prec, 77)
    s = _session(coo, k, prec, A, B)
    try:
        everyone = np.arange(DIMA, dtype=np.uint64)
        ix_all, sc_all = s.topn_batch(everyone, 10, exclude_seen=True, output_score=True)
        ix_rev, sc_rev = s.topn_batch(everyone[::-1].copy(), 10, exclude_seen=True, output_score=True)
        assert np.array_equal(ix_rev[::-1], ix_all) and np.array_equal(sc_rev[::-1], sc_all)
        for u in (0, 5, 63, 64, 1777, 2999):
            ix1, sc1 = s.topn_batch([u], 10, exclude_seen=True, output_score=True)
            assert np.array_equal(ix1[0], ix_all[u]) and np.array_equal(sc1[0], sc_all[u])
            ix3, sc3 = s.topn_batch([u, 11, u, 2000, u], 10, exclude_seen=True, output_score=True)
            for p in (0, 2, 4):
                assert np.array_equal(ix3[p], ix_all[u]) and np.array_equal(sc3[p], sc_all[u])
            assert np.array_equal(ix3[1], ix_all[11]) and np.array_equal(ix3[3], ix_all[2000])
    finally:
        s.close()


def test_ties(prec):
    """3. 200 item rows duplicated at far-apart indices: equal scores straddle item slices and the n-th boundary"""
    k = 50
    coo = _matrix()
    A, B = _factors(DIMA, DIMB, k, prec, 5)
    rng = np.random.default_rng(9)
    B[:200] *= 1.5                         # (so that the duplicated rows are among the best: ties at the top)
    src = np.arange(200)
    dst = DIMB - 1 - rng.choice(12000, 200, replace=False)
    B[dst] = B[src]
    B[dst[:50] - 6000] = B[src[:50]]       # some scores three times
    s = _session(coo, k, prec, A, B)
    try:
        users = _sample_users(rng, 64)
        rows = _score_rows(s, users, DIMB)
        none = [np.empty(0, np.int64)] * len(users)
        for n in (1, 10, 128):
            first = s.topn_batch(users, n, output_score=True)
            _assert_rows(first, users, rows, none, n, "ties")
            for _ in range(4):
                again = s.topn_batch(users, n, output_score=True)
                assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        one = s.topn_batch(users[:3], 7, output_score=True)   # (few users: many item slices)
        _assert_rows(one, users[:3], rows[:3], none[:3], 7, "ties-few")
    finally:
        s.close()


def test_against_float64_truth(prec):
    """4. check_topn (no GPU code in the expectation) for 200 users, the oracle's topn for 20 (fp64: equal indices), and a
    session whose host CSR rows are stored in reversed order"""
    k = 50
    coo = _matrix()
    csr_sp = sp.csr_matrix(coo)
    csr_sp.sum_duplicates(); csr_sp.sort_indices()
    A, B = _factors(DIMA, DIMB, k, prec, 31)
    s = _session(coo, k, prec, A, B)
    rng = np.random.default_rng(2)
    users = _sample_users(rng, 200)
    seen = _rows_of(csr_sp, users)
    none = np.empty(0, np.uint64)
    try:
        ix, sc = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
        for i, u in enumerate(users):
            H.check_topn(A[u], B, ix[i], sc[i], none, seen[i].astype(np.uint64), 10, T(prec, 1e-13, 1e-5))
        ora = bindings.Oracle(prec)
        for i in range(20):
            rc, ixo, sco = ora.topn(A[users[i]], B, none, seen[i].astype(np.uint64), 10)
            assert rc == 0
            if not prec:
                assert np.array_equal(ix[i], ixo)
    finally:
        s.close()
    csr, csc = harness.process_data(coo, prec)
    rev = api.Session(H._reorder_rows(csr, "rev", rng), H._reorder_rows(csc, "rev", rng), DIMA, DIMB, k, prec)
    try:
        rev.set_factors(A, B)
        ix2, sc2 = rev.topn_batch(users, 10, exclude_seen=True, output_score=True)
        assert np.array_equal(ix2, ix) and np.array_equal(sc2, sc)
    finally:
        rev.close()


def test_host_pointer_entry_and_model(prec):
    """5. poismf_hip_topn_batch / PoisMF.topN_batch: the session call's rows, bit for bit"""
    k = 50
    coo = _matrix()
    csr = sp.csr_matrix(coo)
    csr.sum_duplicates(); csr.sort_indices()
    A, B = _factors(DIMA, DIMB, k, prec, 41)
    s = _session(coo, k, prec, A, B)
    m = api.PoisMF(k=k, use_float=prec)
    m.A, m.B, m.nusers, m.nitems, m.is_fitted = A, B, DIMA, DIMB, True
    try:
        rng = np.random.default_rng(6)
        users = _sample_users(rng, 100)
        for n in (10, 128):
            a = s.topn_batch(users, n, exclude_seen=True, output_score=True)
            b = m.topN_batch(users, n, exclude=csr[users], output_score=True)     # (the batch's rows of A only)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        everyone = np.arange(DIMA)
        a = s.topn_batch(everyone, 10, output_score=True)
        b = m.topN_batch(everyone, 10, output_score=True)                         # (all of A goes up)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = m.topN_batch(everyone, 10)
        assert np.array_equal(c[0], a[0]) and c[1].size == 0
    finally:
        s.close()


def test_size_all_users_of_c2_in_one_call():
    """6. 10^5 x 10^5, 10^7 triplets, k = 50, fp32: every user in one call, seen items excluded"""
    n_users = n_items = 10 ** 5
    t = synth.uniform_triplets(n_users, n_items, 10 ** 7, seed=5)
    k = 50
    A, B = _factors(n_users, n_items, k, True, 8)
    s = api.Session.from_coo(t, k, True)
    try:
        s.set_factors(A, B)
        users = np.arange(n_users, dtype=np.uint64)
        ix, sc = s.topn_batch(users, 10, exclude_seen=True, output_score=True)
        X = sp.csr_matrix((np.ones(len(t.row), np.float32), (t.row, t.col)), shape=t.shape)
        X.sum_duplicates(); X.sort_indices()
        hit = np.zeros(n_users, bool)
        for c in range(10):
            hit |= np.asarray(X[np.arange(n_users), ix[:, c].astype(np.int64)]).ravel() != 0
        assert not hit.any(), f"{int(hit.sum())} users were shown an item they have seen"
        rng = np.random.default_rng(1)
        sample = np.sort(rng.choice(n_users, 64, replace=False))
        rows = _score_rows(s, sample, n_items)
        _assert_rows((ix[sample], sc[sample]), sample, rows, _rows_of(X, sample), 10, "size")
    finally:
        s.close()


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))
def test_c_entry_errors_with_a_device(flavour, case):
    """7. rc 2 and nothing written, through the C entry point itself"""
    users, n, excl = BAD[case]
    rc, out, sc = _c_call(flavour, users, n, excl)
    assert rc == 2 and np.all(out == 12345) and np.all(sc == -7.0)


def test_c_entry_valid_call_with_a_device():
    rc, out, sc = _c_call(True, [0, 1, 0], 5, ([0, 2, 2, 3], [0, 1, 4]))
    assert rc == 0
    # all scores are equal (factors of ones): ascending item indices, the user's exclusions left out
    assert out.tolist() == [[2, 3, 4, 5, 6], [0, 1, 2, 3, 4], [0, 1, 2, 3, 5]]
    assert np.all(sc == 3.0)


def test_exclude_seen_outside_the_shard(prec):
    """7. exclude_seen on a session created with a partial shardA, for a user outside it: rc 2 from the library itself"""
    k = 8
    coo = _matrix()
    csr, csc = harness.process_data(coo, prec)
    A, B = _factors(DIMA, DIMB, k, prec, 3)
    s = api.Session(csr, csc, DIMA, DIMB, k, prec, shardA=(1000, 2000), shardB=(0, DIMB))
    try:
        s.set_factors(A, B)
        users = np.array([1500, 2000], np.uint64)
        out = np.full((2, 5), 12345, np.uint64)
        rc = s.lib.poismf_hip_session_topn_batch(s.h, api._ptr(users), 2, 5, 1, None, None, api._ptr(out), None)
        assert rc == 2 and np.all(out == 12345)
        with pytest.raises(ValueError):
            s.topn_batch(users, 5, exclude_seen=True)
        inside = np.array([1000, 1500, 1999], np.uint64)
        ix, sc = s.topn_batch(inside, 5, exclude_seen=True, output_score=True)
        sp_csr = sp.csr_matrix(coo)
        sp_csr.sum_duplicates(); sp_csr.sort_indices()
        rows = _score_rows(s, inside, DIMB)
        _assert_rows((ix, sc), inside, rows, _rows_of(sp_csr, inside), 5, "shard")
        ix2, _ = s.topn_batch(users, 5)            # without exclude_seen any user of A may be asked for
        assert ix2.shape == (2, 5)
    finally:
        s.close()


def test_too_few_items_left_with_exclude_seen():
    """n_top against dimB - |seen U exclude|: refused when the union leaves too few, served when it leaves exactly n_top"""
    dimA, dimB, k = 70, 40, 4
    rng = np.random.default_rng(0)
    dense = np.zeros((dimA, dimB))
    dense[3, :30] = 1          # user 3 has seen items 0..29
    dense[rng.integers(0, dimA, 200), rng.integers(0, dimB, 200)] = 1
    dense[3, 30:] = 0
    coo = sp.coo_matrix(dense)
    A, B = _factors(dimA, dimB, k, True, 1)
    s = _session(coo, k, True, A, B)
    try:
        users = [3, 4]
        overlap = ([0, 8, 8], [22, 23, 24, 25, 26, 27, 28, 29])        # all seen already: 10 items left
        ix, _ = s.topn_batch(users, 10, exclude_seen=True, exclude=overlap)
        assert sorted(ix[0].tolist()) == list(range(30, 40))
        fresh = ([0, 1, 1], [35])                                       # 9 items left
        with pytest.raises(ValueError):
            s.topn_batch(users, 10, exclude_seen=True, exclude=fresh)
    finally:
        s.close()


def test_fitted_model_end_to_end():
    """8. C1: fit, then the top 10 of all 100 users minus their training rows, against float64 truth"""
    coo = synth.readme_coo()
    m = api.PoisMF(k=5, method="cg").fit(coo)
    csr = sp.csr_matrix(coo)
    csr.sum_duplicates(); csr.sort_indices()
    users = np.arange(100)
    ix, sc = m.topN_batch(users, 10, exclude=csr, output_score=True)
    none = np.empty(0, np.uint64)
    for u in users:
        H.check_topn(m.A[u], m.B, ix[u], sc[u], none, csr.indices[csr.indptr[u]:csr.indptr[u + 1]].astype(np.uint64), 10, 1e-5)


def test_lists_exactly_full_across_the_three_tile_kernels(prec):
    """9. The guarded append at a list that is exactly full (tb_select.hpp), through the three kernels that share the selection:
    three users over 300 items, k = 5, scores that rise strictly with the item index, fall strictly, and are all equal (every pass
    appends 16 candidates or none, and the tie rule decides everything).  n_top = 1 gives lists of 1 + 16 + 1 slots -- a prune every
    pass -- and 128 is the deepest.  Three users alone cut the items into several slices; the same three listed 16384 times each make
    768 tiles of users, which is one slice.  Every score is a small integer, so the chains are exact in both precisions and the
    expectation (tests.helpers.check_topn with no tolerance, and the lexsort of the float64 product for the order among ties) has no
    rounding in it.  topn_batch, topn_quota with every quota equal to n_top and the shared table of one list of all items agree bit
    for bit."""
    dimB, k = 300, 5
    dt = H.dtype_of(prec)
    rng = np.random.default_rng(4)
    j = np.arange(dimB)
    r = rng.integers(0, 8, dimB)
    B = np.stack([j + 1, dimB - j, np.ones(dimB), r, 8 - r], axis=1).astype(dt)
    A = np.array([[2, 0, 3, 1, 1], [0, 1, 0, 2, 2], [0, 0, 5, 3, 3]], dt)   # 2 j + 13, 316 - j, 29
    true = B.astype(np.float64) @ A.astype(np.float64).T
    assert np.all(np.diff(true[:, 0]) > 0) and np.all(np.diff(true[:, 1]) < 0) and np.all(true[:, 2] == 29)
    s = _session(sp.coo_matrix((np.ones(3), ([0, 1, 2], [0, 1, 2])), shape=(3, dimB)), k, prec, A, B)
    try:
        everything = (np.array([0, dimB], np.uint64), j.astype(np.uint64))
        none = np.empty(0, np.uint64)
        for users in (np.arange(3, dtype=np.uint64), np.tile(np.arange(3, dtype=np.uint64), 16384)):
            for n in (1, 128):
                plain = s.topn_batch(users, n, output_score=True)
                quota = s.topn_quota(users, n, group_of=j % 4, quota=n, output_score=True)
                shared = s.topn_batch(users, n, include=everything, include_of=0, output_score=True)
                for what, got in (("quota", quota), ("shared", shared)):
                    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), (what, len(users), n)
                ix, sc = plain
                assert ix.shape == (len(users), n) and sc.shape == (len(users), n) and sc.dtype == dt
                for u in range(3):
                    eix, esc = _expect(true[:, u], none, n)
                    assert np.array_equal(ix[u::3], np.broadcast_to(eix, ix[u::3].shape)), (len(users), n, u, ix[u], eix)
                    assert np.array_equal(sc[u::3], np.broadcast_to(esc.astype(dt), sc[u::3].shape)), (len(users), n, u)
                    H.check_topn(A[u], B, ix[u], sc[u], none, none, n, 0.0)
    finally:
        s.close()
