"""Inputs and expectations for the serving calls (include/poismf_hip.h sections 1d, 1f - 1p) on signed, sparse, subnormal, huge and
infinite scores -- numpy only, no GPU code: tests/test_serving_values_cpu.py shows that this file alone meets the conditions
tests/test_gpu_serving_values.py relies on.

The world.  Integer matrices Ai [150 x k] and Bi [3077 x k] with entries in [-3, 3], scaled by powers of two: A = ldexp(Ai, eA),
B = ldexp(Bi, eB) in real_t.  150 users are two full tiles of 64 and a part of a third; 3077 items are 48 full tiles and one with 59
phantom columns.  Every product and every partial sum of a score is an integer below 2^10 in magnitude (k <= 65) times 2^(eA + eB),
so the chain is exact in both precisions and in every summation order, and the expectation of every entry point is

    S = ldexp(Ai @ Bi.T, eA + eB)

with no tolerance anywhere.  Integer scores in [-585, 585] over 3077 items give every user many ties.

Users 0 .. 3 are fixed (in every regime; they override what the regime says about the factors' range):
    0   Ai = 0: every score is 0 and the answer is the index order alone
    1   Ai = (-3, 0, ..., 0): with Bi[:, 0] in {1, 2, 3} every score is negative, in three tie classes of about 1000 items
    2   Ai = (+3, 0, ..., 0): every score positive, in the same classes
    3   its exclusion list EXTRA[3] leaves exactly 128 admissible items (and its seen row lies inside that list)
The other users are random in [-3, 3] with half of the entries zero and a nonzero column 0 (so that at k = 1 their scores are not
all zero); Bi has column 0 in {1, 2, 3} and the other columns in [-3, 3] with half of the entries zero.

Regimes (REGIMES, SCALES):
    signed    as above, unscaled
    sparse    Ai, Bi in [0, 3] with 85 % zeros in every column, column 0 included: thousands of items score exactly 0
    sub_out   normal operands, every product and sum subnormal
    sub_a     subnormal operands on the users' side
    sub_b     subnormal operands on the items' side
    huge      large, no overflow
    overflow  the signed world with column 0 replaced: B[:, 0] = 0 except on the items J (42 of them, spread over the tiles, three in
              the last, partial one), where it is 2^100 (fp64: 2^900); A[:, 0] in {0, +2^100, -2^100}.  A score is +inf or -inf exactly
              where both column-0 entries are nonzero, elsewhere the integer product of the other columns; only column 0 ever gives
              an infinity, so no NaN can arise.
"""
import functools

import numpy as np

from poismf_amd import api

DIMA, DIMB = 150, 3077
REGIMES = ("signed", "sparse", "sub_out", "sub_a", "sub_b", "huge", "overflow")
SUBNORMAL = ("sub_out", "sub_a", "sub_b")
KS = {True: (1, 50, 65), False: (1, 33, 50)}      # [is_float]; 65 / 33: one column into a second LDS chunk, 50: the product's k
# [regime][is_float] = (eA, eB)
SCALES = {
    "signed": {True: (0, 0), False: (0, 0)},
    "sparse": {True: (0, 0), False: (0, 0)},
    "sub_out": {True: (-70, -70), False: (-525, -525)},
    "sub_a": {True: (-140, 0), False: (-1050, 0)},
    "sub_b": {True: (0, -140), False: (0, -1050)},
    "huge": {True: (55, 55), False: (500, 500)},
    "overflow": {True: (0, 0), False: (0, 0)},
}
BIG = {True: 100, False: 900}                      # overflow: column 0 holds 2^BIG
J = np.unique(np.r_[np.arange(7, DIMB, 79), 3072, 3075, 3076])   # the items whose column 0 is 2^BIG in `overflow`
KEEP3 = 128                                        # what user 3's exclusion list leaves
INCLUDE_SIZES = (700, 65, 5, 64, 0, 1)             # length of user u's include list: INCLUDE_SIZES[u % 6]
N_TEST = 12                                        # held-out items per user
CASES = [(r, f, k) for r in REGIMES for f in (True, False) for k in KS[f]]


def case_id(case):
    return f"{case[0]}-{'f32' if case[1] else 'f64'}-k{case[2]}"


def _csr_pair(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int64) for r in rows]) if len(rows) else np.empty(0, np.int64)
    return indptr, flat.astype(np.uint64)


class World:
    """The factors, the exact scores and every list of one (regime, precision, k)."""

    def __init__(self, regime, is_float, k):
        self.regime, self.is_float, self.k = regime, bool(is_float), int(k)
        self.dt = np.float32 if is_float else np.float64
        self.eA, self.eB = SCALES[regime][self.is_float]
        rng = np.random.default_rng(1000 * REGIMES.index(regime) + k)
        self._factors(rng)
        self._lists(np.random.default_rng(77))

    # ---- factors and exact scores ----
    def _factors(self, rng):
        k, dt = self.k, self.dt
        if self.regime == "sparse":
            Ai = rng.integers(1, 4, (DIMA, k)) * (rng.random((DIMA, k)) < 0.15)
            Bi = rng.integers(1, 4, (DIMB, k)) * (rng.random((DIMB, k)) < 0.15)
        else:
            Ai = rng.integers(-3, 4, (DIMA, k)) * (rng.random((DIMA, k)) < 0.5)
            Bi = rng.integers(-3, 4, (DIMB, k)) * (rng.random((DIMB, k)) < 0.5)
            Ai[:, 0] = rng.integers(1, 4, DIMA) * rng.choice([-1, 1], DIMA)
            Bi[:, 0] = rng.integers(1, 4, DIMB)
        Ai[:3] = 0
        Ai[1, 0], Ai[2, 0] = -3, 3
        self.sign0 = None
        if self.regime == "overflow":
            sign0 = rng.integers(-1, 2, DIMA)
            sign0[:4] = (0, -1, 1, -1)
            self.sign0 = sign0
            Ai[:, 0] = 0
            Bi[:, 0] = 0
        self.Ai, self.Bi = Ai.astype(np.int64), Bi.astype(np.int64)
        self.A = np.ldexp(self.Ai.astype(np.float64), self.eA).astype(dt)
        self.B = np.ldexp(self.Bi.astype(np.float64), self.eB).astype(dt)
        self.Ei = self.Ai @ self.Bi.T
        self.S = np.ldexp(self.Ei.astype(np.float64), self.eA + self.eB).astype(dt)
        if self.regime == "overflow":
            big = dt(2.0) ** BIG[self.is_float]
            self.A[:, 0] = sign0 * big
            self.B[J, 0] = big
            inf = np.where(sign0[:, None] > 0, np.inf, -np.inf).astype(dt)
            rows = np.flatnonzero(sign0)
            self.S[np.ix_(rows, J)] = np.broadcast_to(inf[rows], (len(rows), len(J)))
        self.A, self.B = np.ascontiguousarray(self.A), np.ascontiguousarray(self.B)
        # the total order of every user over all items: score descending, item ascending (the cast is exact)
        every = np.arange(DIMB)
        self.order = np.stack([np.lexsort((every, -self.S[u].astype(np.float64))) for u in range(DIMA)])
        self.pos = np.empty_like(self.order)
        np.put_along_axis(self.pos, self.order, np.broadcast_to(every, self.order.shape), axis=1)

    # ---- the lists: the same for every regime, precision and k ----
    def _lists(self, rng):
        every = np.arange(DIMB)
        keep3 = np.union1d(J[::5], [0, 63, 64, 3071, 3076])
        keep3 = np.union1d(keep3, rng.choice(np.setdiff1d(every, keep3), KEEP3 - len(keep3), replace=False))
        self.keep3 = keep3
        seen, extra, incl, test = [], [], [], []
        for u in range(DIMA):
            s = rng.choice(DIMB, 8, replace=False)
            s = np.union1d(s, [J[u % len(J)]])
            e = rng.choice(DIMB, int(rng.integers(0, 300)), replace=False)
            if u % 2:
                e = np.union1d(e, [J[(u + 1) % len(J)], J[(u + 7) % len(J)]])
            if u == 3:
                e = np.setdiff1d(every, keep3)
                s = rng.choice(e, 9, replace=False)
            seen.append(np.unique(s).astype(np.int64))
            extra.append(np.unique(e).astype(np.int64))
            size = INCLUDE_SIZES[u % len(INCLUDE_SIZES)]
            forced = np.array([J[(u + 3) % len(J)], J[(3 * u + 11) % len(J)], 3076, 3073 + u % 3, e[0] if len(e) else 1])[:min(size, 5)]
            forced = np.unique(forced)
            rest = rng.choice(np.setdiff1d(every, forced), size - len(forced), replace=False)
            incl.append(np.union1d(forced, rest).astype(np.int64))
            t = np.r_[e[:3], incl[u][:3], J[(5 * u) % len(J)], J[(u + 3) % len(J)]].astype(np.int64)
            t = np.unique(t)
            t = np.union1d(t, rng.choice(np.setdiff1d(every, t), N_TEST - len(t), replace=False))
            test.append(t.astype(np.int64))
        self.seen, self.extra, self.incl, self.test = seen, extra, incl, test
        self.both = [np.union1d(a, b) for a, b in zip(seen, extra)]
        self.none = [np.empty(0, np.int64)] * DIMA
        # three lists shared between users: all items; 500 with items of J and of the last tile; 70 items
        l1 = np.union1d(np.r_[J[::3], 3070:3077], rng.choice(DIMB, 480, replace=False))
        l2 = np.union1d(np.r_[J[1::7], 5, 3074], rng.choice(DIMB, 60, replace=False))
        self.shared = [every.astype(np.int64), l1.astype(np.int64), l2.astype(np.int64)]
        self.shared_of = (np.arange(DIMA) % 3).astype(np.int64)   # users 0 and 3: all items, 1: l1, 2: l2
        assert all(len(t) == N_TEST for t in test) and len(np.setdiff1d(every, extra[3])) == KEEP3

    def coo(self):
        """the session's own matrix: the seen rows, as a SciPy COO with counts of 1"""
        import scipy.sparse as sp
        row = np.concatenate([np.full(len(s), u) for u, s in enumerate(self.seen)])
        col = np.concatenate(self.seen)
        return sp.coo_matrix((np.ones(len(row)), (row, col)), shape=(DIMA, DIMB))

    def pair(self, rows, users):
        """(indptr, indices) of the users' rows of a per-user list"""
        return _csr_pair([rows[int(u)] for u in users])

    # ---- expectations ----
    def mask(self, users, include=None, exclude=None, unite=None):
        """[m x DIMB] bool: C(u) = (include(u), or every item; united with unite(u)) minus exclude(u), rows given per entry of `users`"""
        m = np.zeros((len(users), DIMB), bool)
        for i in range(len(users)):
            if include is None:
                m[i] = True
            else:
                m[i, include[i]] = True
            if unite is not None:
                m[i, unite[i]] = True
            if exclude is not None:
                m[i, exclude[i]] = False
        return m

    def topn(self, users, mask, n):
        """items uint64 [m x n] and scores [m x n]: the first n admissible items of each user in the total order, padded with
        TOPN_NONE and -inf"""
        ix = np.full((len(users), n), api.TOPN_NONE, np.uint64)
        sc = np.full((len(users), n), -np.inf, self.dt)
        for i, u in enumerate(users):
            o = self.order[int(u)]
            o = o[mask[i, o]][:n]
            ix[i, :len(o)] = o
            sc[i, :len(o)] = self.S[int(u), o]
        return ix, sc

    def ranks(self, users, mask, tests):
        """(ranks uint32, one per cell in row order: the admissible items before t in the total order, RANK_EXCLUDED for a cell
        that is not admissible; n_adm uint32 [m])"""
        out = []
        for i, u in enumerate(users):
            o = self.order[int(u)]
            before = np.cumsum(mask[i, o]) - mask[i, o]          # admissible items before each position
            t = np.asarray(tests[i], np.int64)
            r = before[self.pos[int(u), t]].astype(np.uint32)
            r[~mask[i, t]] = api.RANK_EXCLUDED
            out.append(r)
        return np.concatenate(out) if out else np.empty(0, np.uint32), mask.sum(axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=3)
def world(regime, is_float, k):
    return World(regime, is_float, k)


def bits(a):
    """a real array as unsigned integers of its width: equality of bits, -0 apart from +0"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
