"""Batched re-rank (include/poismf_hip.h section 1s) on the GPU: every row of every call against a plain reference, bit for bit.

The expectation is built from Session.predict on the (user, candidate) pairs -- the pair_dot_kernel path, which the new kernels do
not share: the scores restricted to I(u) \\ E(u) and ordered by np.lexsort((item, -score)).  np.array_equal on row pointers, items and
score bits: no tolerance and no row left out.  One more case takes world and expectation from tests/serving_values.py, where the
expectation contains no GPU code at all.  Row lengths come from the library's two aids: W = the longest row one wave orders, R = the
entries one workgroup orders."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api
from tests import serving_values as SV

pytestmark = pytest.mark.gpu

DIMB = 65536 + 7
CASES = [(f, k) for f in (True, False) for k in SV.KS[f]]
MODES = ("none", "seen", "list", "both")


class _World:
    """one user per row length, factors with ties, seen items and exclusion lists, the session and the reference scores -- built
    once per (precision, k) and never changed"""

    def __init__(self, is_float, k):
        lib = api.load_library(is_float)
        W, R = int(lib.poismf_hip_order_include_wave_row()), int(lib.poismf_hip_order_include_run())
        self.lengths = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, R - 1, R, R + 1, 2 * R + 1, 3 * R + 5, 65536, R + 1, 3 * R + 5]
        m, rng, dt = len(self.lengths), np.random.default_rng(5 + k), np.float32 if is_float else np.float64
        self.is_float, self.k, self.dimA = is_float, k, m + 3
        self.users = rng.permutation(self.dimA)[:m].astype(np.uint64)
        self.A = rng.standard_normal((self.dimA, k)).astype(dt)
        self.A[self.users[-2:].astype(np.int64)] = 0        # every score ties: the answer is the list itself (lengths R + 1 and 3 R + 5)
        # runs of three equal rows of B: equal scores side by side in every list, across every boundary between runs of R candidates
        self.B = np.ascontiguousarray(rng.standard_normal((DIMB // 3 + 1, k)).astype(dt)[np.arange(DIMB) // 3])
        self.lists = [np.sort(rng.choice(DIMB, ln, replace=False)) for ln in self.lengths]
        # seen: about a fifth of a list and 40 items outside it; the whole list at lengths 2 and 65 (count 0)
        self.seen = [np.union1d(l if len(l) in (2, 65) else l[rng.random(len(l)) < 0.2], rng.choice(DIMB, 40)) for l in self.lists]
        row = np.concatenate([np.full(len(s), int(u)) for u, s in zip(self.users, self.seen)])
        coo = sp.coo_matrix((np.ones(len(row)), (row, np.concatenate(self.seen))), shape=(self.dimA, DIMB))
        self.s = api.Session.from_coo(coo, k, is_float)
        self.s.set_factors(self.A, self.B)
        sizes = np.cumsum(self.lengths)[:-1]
        flat = self.s.predict(np.repeat(self.users, self.lengths), np.concatenate(self.lists).astype(np.uint64))
        self.cell = np.split(flat, sizes)
        # exclusion lists: a tenth of a list and 30 items outside it; the whole list at length 63; at W + 1 exactly the best and the last
        self.extra = [np.union1d(l if len(l) == 63 else l[rng.random(len(l)) < 0.1], rng.choice(DIMB, 30)) for l in self.lists]
        i = self.i_cut = self.lengths.index(W + 1)
        self.extra[i] = np.sort(self.lists[i][np.lexsort((self.lists[i], -self.cell[i].astype(np.float64)))[[0, -1]]])
        self.excluded = {"none": [np.empty(0, np.int64)] * m, "seen": self.seen, "list": self.extra,
                         "both": [np.union1d(a, b) for a, b in zip(self.seen, self.extra)]}

    def expect(self, rows, mode):
        """(indptr, items, scores) of the rows' answers"""
        ix, sc = [], []
        for i in rows:
            keep = ~np.isin(self.lists[i], self.excluded[mode][i])
            idx, s = self.lists[i][keep], self.cell[i][keep]
            o = np.lexsort((idx, -s.astype(np.float64)))   # (the cast is exact; it only keeps -s in one dtype)
            ix.append(idx[o].astype(np.uint64))
            sc.append(s[o])
        return np.concatenate(([0], np.cumsum([len(r) for r in ix]))), np.concatenate(ix), np.concatenate(sc)

    def call(self, rows, mode, target=None):
        kw = dict(exclude=SV._csr_pair([self.extra[i] for i in rows]) if mode in ("list", "both") else None, output_score=True)
        if target is None:
            target, kw["exclude_seen"] = self.s, mode in ("seen", "both")
        return target.order_candidates(self.users[rows], SV._csr_pair([self.lists[i] for i in rows]), **kw)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(SV.bits(got[2]), SV.bits(want[2]))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{'f32' if c[0] else 'f64'}-k{c[1]}")
def w(request):
    return _World(*request.param)


@pytest.mark.parametrize("mode", MODES)
def test_whole_batch_against_predict_and_lexsort(w, mode):
    rows = list(range(len(w.lengths)))
    got, want = w.call(rows, mode), w.expect(rows, mode)
    counts = np.diff(want[0])
    if mode == "list":
        assert counts[w.lengths.index(63)] == 0 and counts[w.i_cut] == w.lengths[w.i_cut] - 2
    if mode == "none":
        assert np.array_equal(got[1][got[0][-3]:got[0][-2]], w.lists[-2].astype(np.uint64))   # A[u] = 0: the list itself
    assert same(got, want)


def test_a_row_does_not_depend_on_its_batch_or_entry_point(w):
    rows = list(range(len(w.lengths)))
    assert same(w.call(rows[::-1], "both"), w.expect(rows[::-1], "both"))
    for i in rows:
        assert same(w.call([i], "both"), w.expect([i], "both")), w.lengths[i]
    model = api.PoisMF(k=w.k, use_float=w.is_float)
    model.A, model.B, model.nusers, model.nitems, model.is_fitted = w.A, w.B, w.dimA, DIMB, True
    assert same(w.call(rows, "list", model), w.expect(rows, "list"))


def test_first_128_are_the_include_top_n(w):
    rows = list(range(len(w.lengths)))
    indptr, items, scores = w.call(rows, "both")
    ix, sc = w.s.topn_batch(w.users, 128, exclude_seen=True, exclude=SV._csr_pair(w.extra), output_score=True, include=SV._csr_pair(w.lists))
    for i in rows:
        n = min(128, indptr[i + 1] - indptr[i])
        assert np.array_equal(ix[i, :n], items[indptr[i]:indptr[i] + n]) and np.all(ix[i, n:] == api.TOPN_NONE), w.lengths[i]
        assert np.array_equal(SV.bits(sc[i, :n]), SV.bits(scores[indptr[i]:indptr[i] + n]))


@pytest.mark.parametrize("case", [c for c in SV.CASES if c[0] in ("signed", "sub_out")], ids=SV.case_id)
def test_serving_values_world(case):
    """expectation without any GPU code: exact integer scores scaled by powers of two; user 0's list is the whole catalogue, whose
    first 1024 are also Session.topn_deep's"""
    v = SV.world(*case)
    s = api.Session.from_coo(v.coo(), v.k, v.is_float)
    s.set_factors(v.A, v.B)
    users = np.arange(SV.DIMA, dtype=np.uint64)
    incl = [np.arange(SV.DIMB)] + v.incl[1:]
    for exclude_seen, lists in ((False, v.none), (True, v.both)):
        mask = v.mask(users, incl, lists)
        got = s.order_candidates(users, SV._csr_pair(incl), exclude_seen=exclude_seen, exclude=SV._csr_pair(v.extra) if exclude_seen else None,
                                 output_score=True)
        order = [v.order[u][mask[u, v.order[u]]] for u in range(SV.DIMA)]
        want = (np.concatenate(([0], np.cumsum([len(o) for o in order]))), np.concatenate(order).astype(np.uint64),
                np.concatenate([v.S[u, o] for u, o in enumerate(order)]))
        assert same(got, want)
        deep = s.topn_deep(users[:1], 1024, exclude_seen=exclude_seen, exclude=SV._csr_pair(v.extra[:1]) if exclude_seen else None, output_score=True)
        assert np.array_equal(deep[0][0], got[1][:1024]) and np.array_equal(SV.bits(deep[1][0]), SV.bits(got[2][:1024]))
