"""What the COO conversion must store, restated in numpy (include/poismf_hip.h section 1c): a cell's value is the sum of its triplets in
the order the caller gave them, s = t1; s = s + t2; s = s + t3; ..., every addition rounded in real_t -- a function of the cell's own
triplets and of nothing else.  No device and no SciPy in any expectation here: coo.tocsr() sorts a row's indices with an unstable sort
on the column alone, so SciPy's order of equal columns is not defined.  Shared by tests/test_coo_values_cpu.py and
tests/test_gpu_coo_values.py."""
import math

import numpy as np

LOOP_MAX = 64   # runs of up to this many triplets are summed by duplicate rank, vectorised over runs; longer ones by np.add.accumulate


class Triplets:
    """row / col / data / shape / nnz: what poismf_amd.api reads of a COO matrix"""

    def __init__(self, row, col, data, shape):
        self.row, self.col, self.data, self.shape = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(data), tuple(shape)
        self.nnz = len(self.data)


def _sorted_runs(row, col, val, shape, dt, major, lo, hi):
    """the triplets of major rows [lo, hi) in a stable (major, minor) order: (major - lo, minor, values in dt, start of every run, the
    runs' lengths, number of major rows)"""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    val = np.asarray(val, dt)
    maj, mnr = (row, col) if major == 0 else (col, row)
    dim = shape[0] if major == 0 else shape[1]
    lo, hi = (0 if lo is None else lo), (dim if hi is None else hi)
    keep = (maj >= lo) & (maj < hi)
    maj, mnr, val = maj[keep] - lo, mnr[keep], val[keep]
    order = np.lexsort((mnr, maj))   # stable: equal cells stay in input order
    maj, mnr, val = maj[order], mnr[order], val[order]
    head = np.ones(len(val), bool)
    head[1:] = (maj[1:] != maj[:-1]) | (mnr[1:] != mnr[:-1])
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, len(val)))
    return maj, mnr, val, start, length, hi - lo


def reference_cs(row, col, val, shape, dt, major, lo=None, hi=None, loop_max=LOOP_MAX):
    """(values, indices, indptr) of one orientation -- major = 0: the CSR, major = 1: the CSC -- under the sequential rule.  With lo, hi:
    the major rows [lo, hi) only, indptr local from 0.  values in dt, indices and indptr int64."""
    maj, mnr, val, start, length, dim = _sorted_runs(row, col, val, shape, dt, major, lo, hi)
    s = val[start].copy()
    short = length <= loop_max
    for r in range(1, int(min(length.max(initial=1), loop_max))):
        sel = np.flatnonzero(short & (length > r))
        s[sel] = s[sel] + val[start[sel] + r]          # one rounded addition in dt
    for c in np.flatnonzero(~short):
        s[c] = np.add.accumulate(val[start[c]:start[c] + length[c]], dtype=dt)[-1]
    assert s.dtype == np.dtype(dt)
    indptr = np.zeros(dim + 1, np.int64)
    np.cumsum(np.bincount(maj[start], minlength=dim), out=indptr[1:])
    return s, mnr[start].copy(), indptr


def exact_and_bound(row, col, val, shape, dt, major=0, lo=None, hi=None, got=None):
    """Per cell, in reference_cs's order: the sum of its triplets by math.fsum, and the bound (d - 1) * u * fsum(|t|), u = eps / 2, that
    the rounded sum of d terms meets in ANY order (Rump 2012: no higher-order terms are needed) -- derived, not measured.  With `got`
    (a candidate's values), a third array: |got - exact sum| over the bound (0 where the bound is 0: a lone triplet must be stored as it
    is), the difference taken by fsum over the candidate and the negated terms, so it is rounded once, relative to itself."""
    _, _, v, start, length, _ = _sorted_runs(row, col, val, shape, dt, major, lo, hi)
    u = float(np.finfo(dt).eps) / 2
    exact, bound = np.empty(len(start)), np.empty(len(start))
    ratio = None if got is None else np.zeros(len(start))
    for c, (a, d) in enumerate(zip(start.tolist(), length.tolist())):
        t = v[a:a + d].astype(np.float64).tolist()
        exact[c] = math.fsum(t)
        bound[c] = (d - 1) * u * math.fsum(abs(x) for x in t)
        if got is not None:
            err = abs(math.fsum([float(got[c])] + [-x for x in t]))
            ratio[c] = err / bound[c] if bound[c] > 0 else (0.0 if err == 0 else math.inf)
    return (exact, bound) if got is None else (exact, bound, ratio)


def big_of(dt):
    """the power of two from which on dt's spacing is 2: adding 1 to it is absorbed (round to even)"""
    return dt(2.0 ** 24) if dt == np.float32 else dt(2.0 ** 53)


def absorption_triplets(dt):
    """two cells of one call, their triplets interleaved: (2, 1) given as (big, 1, 1), which stays big, and (0, 3) given as
    (1, 1, big), which is big + 2"""
    big = big_of(dt)
    return Triplets([2, 0, 2, 0, 0, 2], [1, 3, 1, 3, 3, 1], np.array([big, 1, 1, 1, big, 1], dt), (4, 5))


SHAPE = (300, 200)     # rows 290..299 and columns 190..199 stay empty
N_MANY, N_TWO, N_ONE = 4000, 4000, 6000


def world(dt, seed):
    """Triplets of a 300 x 200 matrix: 4000 cells with 3..40 triplets each, 4000 with two, 6000 with one, values uniform(0.1, 9.0)
    cast to dt, shuffled by a fixed permutation: about 100 000 triplets."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(290 * 190, size=N_MANY + N_TWO + N_ONE, replace=False)
    r, c = cells // 190, cells % 190
    count = np.concatenate([rng.integers(3, 41, N_MANY), np.full(N_TWO, 2), np.full(N_ONE, 1)])
    row, col = np.repeat(r, count), np.repeat(c, count)
    val = rng.uniform(0.1, 9.0, len(row)).astype(dt)
    order = rng.permutation(len(row))
    return Triplets(row[order], col[order], val[order], SHAPE)


def cell_counts(t, major=0):
    """number of triplets of every cell of t, in reference_cs's order"""
    return _sorted_runs(t.row, t.col, t.data, t.shape, t.data.dtype, major, None, None)[4]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
