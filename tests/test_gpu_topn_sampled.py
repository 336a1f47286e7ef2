"""The sampled top-N (include/poismf_hip.h section 1w) on the GPU against a numpy reference of its definition: Philox4x32-10 in uint64
arithmetic, float64 log1p and power, and predict's score bits -- so what is judged is the factor and the selection, not the chain.

A user's page must equal the reference page wherever every pair of adjacent reference keys up to the boundary pair (n, n + 1) differs by
more than EPS_R relative: the device makes the factor in real_t, and EPS_R is four times the largest relative error of its keys measured
over these very cases.  At most 5 % of a case's users may be left out as too close.

No id of 2^32 or more appears: a stream is named by a row of A, and every entry point refuses dimA above 2^31 - 1."""
import numpy as np
import pytest

from poismf_amd import api
from tests import helpers as H
from tests.test_gpu_topn_deep import _excl_pair, _session
from tests.test_gpu_topn_weighted import _model

pytestmark = pytest.mark.gpu

MASK = np.uint64(2 ** 32 - 1)
EPS_R = {True: 4 * 6.0e-7, False: 4 * 1.04e-15}   # use_float -> bound; measured over these cases: 5.96e-7 / 1.04e-15, both at T = 3
# a seed under which the float64 reference alone leaves out at most 3 of the 70 users (4.3 %) in every case below at these bounds
N_USERS, SEED = 70, 0xDAA66D2C7DDF743F


@pytest.fixture(scope="module", params=[False, True], ids=["f64", "f32"])
def prec(request):
    return request.param


def words(seed, users, dimB):
    """word(u, j) of the definition, [len(users) x dimB]"""
    j = np.arange(dimB, dtype=np.uint64)[None, :]
    u = np.asarray(users, np.uint64)[:, None]
    c = [(j >> np.uint64(2)) + 0 * u, 1 + 0 * (u + j), (u & MASK) + 0 * j, (u >> np.uint64(32)) + 0 * j]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.take_along_axis(np.stack(c), (j & np.uint64(3)).astype(np.int64)[None] + 0 * u.astype(np.int64)[None], axis=0)[0]


def ref_keys(scores, seed, users, T):
    """float64 keys [m x dimB]: predict's score bits times E^(-T)"""
    V = (words(seed, users, scores.shape[1]).astype(np.float64) + 0.5) / 2.0 ** 32
    return scores.astype(np.float64) * np.power(-np.log1p(-V), -T)


def ref_pages(keys, excl, n, eps):
    """(pages [m x n] padded with TOPN_NONE, clear [m]: every adjacent pair of keys up to (n, n + 1) is further apart than eps relative)"""
    pages, clear = np.full((len(keys), n), api.TOPN_NONE, np.uint64), np.ones(len(keys), bool)
    for i, row in enumerate(keys):
        idx = np.setdiff1d(np.arange(len(row)), excl[i])
        o = idx[np.lexsort((idx, -row[idx]))][:n + 1]
        pages[i, :min(n, len(o))] = o[:n]
        k = row[o]
        clear[i] = bool(np.all(k[:-1] - k[1:] > eps * k[:-1]))
    return pages, clear


def users_of(dimA, m=N_USERS):
    """m distinct rows of A spread over all of it, the last row among them, in no order"""
    u = np.unique(np.concatenate((np.random.default_rng(5).integers(0, dimA, 2 * m), [dimA - 1])))[-m:]
    return np.random.default_rng(6).permutation(u).astype(np.uint64)


def world(dimA, dimB, k, prec, users, seed):
    """a model whose factor rows are random for `users` and zero elsewhere, and the users' score rows from the predict path"""
    rng, dt = np.random.default_rng(seed), H.dtype_of(prec)
    A, B, rows = np.zeros((dimA, k), dt), rng.random((dimB, k)).astype(dt), rng.random((len(users), k)).astype(dt)
    A[users.astype(np.int64)] = rows
    scores = np.empty(len(users) * dimB, dt)
    api._predict_multiple(scores, rows, B, np.repeat(np.arange(len(users), dtype=np.uint64), dimB), np.tile(np.arange(dimB, dtype=np.uint64), len(users)))
    return _model(A, B, k, prec), scores.reshape(len(users), dimB)


@pytest.mark.parametrize("k", (1, 16, 50, 65))
def test_pages_scores_and_keys(prec, k):
    """1. and 2.: items against the reference page, scores against predict's bits, keys within EPS_R, padding where a row is short"""
    dimA = 2 ** 28 // k      # (A is 2 GiB of untouched zeros in double; the ids reach bit 27 of the low counter word at k = 1)
    users = users_of(dimA)
    worst, left_out = 0.0, 0.0
    for dimB in (3, 64, 67, 1000):
        m, scores = world(dimA, dimB, k, prec, users, 100 * k + dimB)
        rng = np.random.default_rng(dimB)
        lists = [np.flatnonzero(rng.random(dimB) < 0.3) for _ in users]
        for T in (0.5, 1.0, 3.0):
            keys = ref_keys(scores, SEED + dimB, users, T)
            for excl in (None, lists):
                rows = excl if excl else [np.empty(0, np.int64)] * len(users)
                for n in (1, 10, 128):
                    want, clear = ref_pages(keys, rows, n, EPS_R[prec])
                    ix, sc, ky = m.topN_sampled(users, n, T, SEED + dimB, exclude=_excl_pair(excl) if excl else None, output_score=True,
                                                output_key=True)
                    left_out = max(left_out, 1 - clear.mean())
                    assert clear.mean() >= 0.95, (dimB, T, n, "too many users too close to call")
                    assert np.array_equal(ix[clear], want[clear]), (dimB, T, n, excl is not None)
                    real = ix != api.TOPN_NONE
                    at = np.nonzero(real)
                    assert np.all(real.sum(axis=1) == [min(n, dimB - len(r)) for r in rows])
                    assert sc[real].tobytes() == scores[at[0], ix[real].astype(np.int64)].tobytes()
                    assert np.all(np.isneginf(sc[~real])) and np.all(np.isneginf(ky[~real]))
                    exact = keys[at[0], ix[real].astype(np.int64)]
                    worst = max(worst, float(np.max(np.abs(ky[real] - exact) / exact, initial=0.0)))
    print(f"k {k} f32 {prec}: largest relative key error {worst:.3e}, most users left out {left_out:.3f}")
    assert worst <= EPS_R[prec]


@pytest.mark.parametrize("seed", (0, 7, 2 ** 63 + 11))
def test_temperature_zero_is_the_plain_call(prec, seed):
    """3.: items and score bits of topn_batch, for any seed; the keys are the scores"""
    A, B = (np.random.default_rng(3).random(s).astype(H.dtype_of(prec)) for s in ((130, 50), (1000, 50)))
    s = _session(130, 1000, 50, prec, A, B)
    try:
        users = np.arange(130, dtype=np.uint64)
        for n in (1, 10, 128):
            ix, sc = s.topn_batch(users, n, exclude_seen=True, output_score=True)
            got = s.topn_sampled(users, n, 0.0, seed, exclude_seen=True, output_score=True, output_key=True)
            assert np.array_equal(got[0], ix) and got[1].tobytes() == sc.tobytes() and got[2].tobytes() == sc.tobytes()
    finally:
        s.close()


def test_a_row_depends_on_its_user_alone(prec):
    """4.: alone, in a batch of 200 and elsewhere in it (16 item slices each); in a batch of 17 600 (3 item slices) and across its chunk
    boundary, which more exclusion indices than one chunk's area holds (2^24) force; the session against the host-pointer call; the same
    seed again, and another"""
    dimA, dimB, k, n = 300, 1000, 50, 10
    rng, dt = np.random.default_rng(11), H.dtype_of(prec)
    A, B = rng.random((dimA, k)).astype(dt), rng.random((dimB, k)).astype(dt)
    s = _session(dimA, dimB, k, prec, A, B)
    try:
        batch = rng.permutation(dimA)[:200].astype(np.uint64)
        kw = dict(temperature=1.0, seed=99, output_score=True, output_key=True)
        whole = s.topn_sampled(batch, n, **kw)
        for got in (s.topn_sampled(batch[::-1].copy(), n, **kw), _model(A, B, k, prec).topN_sampled(batch[::-1].copy(), n, **kw)):
            assert all(g[::-1].tobytes() == w.tobytes() for g, w in zip(got, whole))
        for i in (0, 77, 199):
            assert all(g.tobytes() == w[i:i + 1].tobytes() for g, w in zip(s.topn_sampled(batch[i:i + 1], n, **kw), whole))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(s.topn_sampled(batch, n, **kw), whole))
        assert (s.topn_sampled(batch, n, **{**kw, "seed": 100})[0] != whole[0]).any(axis=1).mean() > 0.9
        # 17 600 rows of 960 excluded items: two chunks; the rows on either side of the cut against the same rows in a small batch
        m, keep = 17600, np.arange(40) * 25
        row = np.setdiff1d(np.arange(dimB), keep).astype(np.uint64)
        assert m * len(row) > api.TOPN_SAMPLED_MAX_ITEMS
        many = np.resize(batch, m)
        big = s.topn_sampled(many, n, exclude=(np.arange(m + 1, dtype=np.uint64) * len(row), np.tile(row, m)), **kw)
        small = s.topn_sampled(batch, n, exclude=(np.arange(201, dtype=np.uint64) * len(row), np.tile(row, 200)), **kw)
        assert np.isin(small[0], keep).all()
        for lo in (0, 17390):
            assert all(b[lo:lo + 200].tobytes() == np.roll(w, -(lo % 200), axis=0).tobytes() for b, w in zip(big, small))
    finally:
        s.close()


def test_the_draw_follows_the_scores():
    """5.: two items with scores 1 and 3, n = 1, T = 1, 4096 users with equal factor rows: the item of score 3 is drawn about 3072 times"""
    m = 4096
    A, B = np.ones((m, 1), np.float32), np.array([[1.0], [3.0]], np.float32)
    users = np.arange(m, dtype=np.uint64)
    keys = ref_keys(np.tile(B.T, (m, 1)), 2024, users, 1.0)
    device = int(_model(A, B, 1, True).topN_sampled(users, 1, 1.0, 2024)[0].sum())
    reference = int((keys[:, 1] > keys[:, 0]).sum())
    print(f"the item of score 3 is drawn {device} times on the device, {reference} times by the reference")
    bound = 5 * np.sqrt(m * 0.75 * 0.25)
    assert abs(device - 3072) <= bound and abs(reference - 3072) <= bound
