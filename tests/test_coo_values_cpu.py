"""The reference of the COO conversion's values (tests/coo_values.py) checked by hand, the power of its test world, and what
poismf_hip_coo_to_csr_csc refuses before any device work (include/poismf_hip.h section 1c).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from poismf_amd import api
from tests import coo_values as V
from tests.coo_values import bits, reference_cs

PRECS = pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])


# ---- hand-written answers ----------------------------------------------------------------------------------------------------------
@PRECS
def test_absorption_follows_the_input_order(dt):
    t = V.absorption_triplets(dt)
    big = V.big_of(dt)
    val, ind, ptr = reference_cs(t.row, t.col, t.data, t.shape, dt, 0)
    assert val.dtype == dt and val.tolist() == [float(big) + 2.0, float(big)]     # (1 + 1) + big; (big + 1) + 1 = big
    assert ind.tolist() == [3, 1] and ptr.tolist() == [0, 1, 1, 2, 2]
    val, ind, ptr = reference_cs(t.row, t.col, t.data, t.shape, dt, 1)
    assert val.tolist() == [float(big), float(big) + 2.0]
    assert ind.tolist() == [2, 0] and ptr.tolist() == [0, 0, 1, 1, 2, 2]


@PRECS
def test_lone_triplet_empty_rows_and_the_cut(dt):
    # rows 0 and 5 empty (both ends), row 1: cells 4 (twice) and 0, row 3: cell 2 alone, row 4: cell 2 three times
    row = [4, 1, 3, 1, 4, 1, 4]
    col = [2, 4, 2, 0, 2, 4, 2]
    val = np.array([0.5, 0.25, 7.0, 3.0, 0.125, 1.0, 2.0], dt)
    full = reference_cs(row, col, val, (6, 5), dt, 0)
    assert full[0].tolist() == [3.0, 1.25, 7.0, 2.625] and full[1].tolist() == [0, 4, 2, 2] and full[2].tolist() == [0, 0, 2, 2, 3, 4, 4]
    csc = reference_cs(row, col, val, (6, 5), dt, 1)
    assert csc[0].tolist() == [3.0, 7.0, 2.625, 1.25] and csc[1].tolist() == [1, 3, 4, 1] and csc[2].tolist() == [0, 1, 1, 3, 3, 4]
    cut = reference_cs(row, col, val, (6, 5), dt, 0, 3, 5)
    assert cut[0].tolist() == [7.0, 2.625] and cut[1].tolist() == [2, 2] and cut[2].tolist() == [0, 1, 2]
    cut = reference_cs(row, col, val, (6, 5), dt, 0, 2, 3)                       # a cut that holds no triplet
    assert len(cut[0]) == 0 and len(cut[1]) == 0 and cut[2].tolist() == [0, 0]
    cut = reference_cs(row, col, val, (6, 5), dt, 1, 2, 5)                       # columns 2, 3, 4
    assert cut[0].tolist() == [7.0, 2.625, 1.25] and cut[1].tolist() == [3, 4, 1] and cut[2].tolist() == [0, 2, 2, 3]
    for (lo, hi) in ((0, 1), (1, 4), (5, 6)):
        a, b = full[2][lo], full[2][hi]
        cut = reference_cs(row, col, val, (6, 5), dt, 0, lo, hi)
        assert np.array_equal(bits(cut[0]), bits(full[0][a:b])) and np.array_equal(cut[1], full[1][a:b])
        assert np.array_equal(cut[2], full[2][lo:hi + 1] - a)


@PRECS
def test_rank_loop_and_accumulate_agree(dt):
    rng = np.random.default_rng(5)
    n = 65
    val = rng.uniform(0.1, 9.0, 3 * n).astype(dt)
    row, col = np.tile([1, 0, 1], n), np.tile([2, 0, 2], n)                       # cell (1, 2): 130 triplets, cell (0, 0): 65
    by_rank = reference_cs(row, col, val, (2, 3), dt, 0, loop_max=1000)
    by_accumulate = reference_cs(row, col, val, (2, 3), dt, 0)
    mixed = reference_cs(row, col, val, (2, 3), dt, 0, loop_max=65)
    s = val[1::3][0]
    for x in val[1::3][1:]:
        s = dt(s + x)
    assert bits(by_rank[0])[0] == bits(np.array([s], dt))[0]
    for other in (by_accumulate, mixed):
        assert np.array_equal(bits(other[0]), bits(by_rank[0])) and np.array_equal(other[1], by_rank[1]) and np.array_equal(other[2], by_rank[2])


# ---- the world can tell one order of summation from another -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def world_ref(request):
    dt = request.param
    w = V.world(dt, 11)
    return dt, w, reference_cs(w.row, w.col, w.data, w.shape, dt, 0), V.cell_counts(w)


def test_world_is_what_it_says(world_ref):
    dt, w, ref, count = world_ref
    assert w.shape == (300, 200) and w.data.dtype == dt and 95000 < w.nnz < 112000
    assert w.row.max() < 290 and w.col.max() < 190
    assert (count >= 3).sum() == 4000 and count.max() == 40 and (count == 2).sum() == 4000 and (count == 1).sum() == 6000
    assert np.any(np.diff(w.row * 200 + w.col) < 0)                              # shuffled
    assert np.array_equal(ref[2][290:], np.full(11, len(ref[0])))


def test_world_has_power(world_ref):
    dt, w, ref, count = world_ref
    many = count >= 3
    rev = reference_cs(w.row[::-1], w.col[::-1], w.data[::-1], w.shape, dt, 0)   # every cell's triplets reversed
    assert np.array_equal(rev[1], ref[1]) and np.array_equal(rev[2], ref[2])
    changed = (bits(rev[0]) != bits(ref[0]))[many].mean()
    print(f"reversed: {changed:.3f} of the cells with >= 3 triplets change")
    assert changed >= 0.40
    # t1 + (t2 + t3 + ...): the first triplet of every cell is taken out, the rest summed by the rule, then one addition
    key = w.row * 200 + w.col
    first = np.zeros(w.nnz, bool)
    first[np.unique(key, return_index=True)[1]] = True
    tail = reference_cs(w.row[~first], w.col[~first], w.data[~first], w.shape, dt, 0)
    order = np.argsort(key[first], kind="stable")
    t1 = w.data[first][order]                                                    # in cell order
    assert np.array_equal(np.sort(key[first]), np.unique(key)) and len(tail[0]) == (count >= 2).sum()
    alt = ref[0].copy()
    alt[count >= 2] = t1[count >= 2] + tail[0]
    assert np.array_equal(bits(alt[count == 2]), bits(ref[0][count == 2]))       # (two terms: nothing to re-associate)
    changed = (bits(alt) != bits(ref[0]))[many].mean()
    print(f"re-associated: {changed:.3f} of the cells with >= 3 triplets change")
    assert changed >= 0.25


def test_reference_meets_its_own_bound(world_ref):
    dt, w, ref, count = world_ref
    exact, bound, ratio = V.exact_and_bound(w.row, w.col, w.data, w.shape, dt, 0, got=ref[0])
    assert len(exact) == len(ref[0]) and np.all(bound[count == 1] == 0) and np.all(bound[count > 1] > 0)
    assert np.array_equal(bits(ref[0][count == 1]), bits(exact[count == 1].astype(dt)))
    print(f"worst |reference - exact| / bound: {ratio.max():.3f}")
    assert ratio.max() <= 1.0


# ---- refusals of poismf_hip_coo_to_csr_csc ------------------------------------------------------------------------------------------
DIMA, DIMB = 7, 5
BAD = {
    "row-is-dimA": ([0, DIMA, 1], [0, 1, 2]),
    "col-is-dimB": ([0, 1, 2], [0, 1, DIMB]),
    "row-2^32+3": ([0, 2 ** 32 + 3, 1], [0, 1, 2]),
    "col-2^32+3": ([0, 1, 2], [2 ** 32 + 3, 1, 2]),
    "row-negative": ([0, 1, -1], [0, 1, 2]),
    "col-negative": ([-2, 1, 2], [0, 1, 2]),
}


def _cases(flavour):
    # (the R flavour's int cannot hold 2^32 + 3; a negative size_t is the huge index it reads as, kept for all three)
    return sorted(c for c in BAD if not (flavour == "r" and "2^32" in c))


def _c_call(flavour, row, col):
    """poismf_hip_coo_to_csr_csc itself through ctypes; index arrays in the flavour's sparse_ix"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    r, c = ix(row), ix(col)
    n = len(r)
    val = np.full(n, 1.5, dt)
    outs = [np.full(n, -7.0, dt), np.full(n, 12345, it), np.full(DIMA + 1, 12345, it),
            np.full(n, -7.0, dt), np.full(n, 12345, it), np.full(DIMB + 1, 12345, it)]
    nnz = C.c_size_t(4321)
    p = api._ptr
    rc = lib.poismf_hip_coo_to_csr_csc(p(r), p(c), p(val), n, DIMA, DIMB, *[p(o) for o in outs], C.byref(nnz))
    return rc, outs, nnz.value


@pytest.mark.parametrize("flavour,case", [pytest.param(f, c, id=f"{name}-{c}") for f, name in ((False, "d"), (True, "f"), ("r", "r"))
                                          for c in _cases(f)])
def test_c_entry_returns_3_and_writes_nothing(flavour, case):
    rc, outs, nnz = _c_call(flavour, *BAD[case])
    assert rc == 3
    assert all(np.all(o == (-7.0 if o.dtype.kind == "f" else 12345)) for o in outs) and nnz == 4321


@pytest.mark.parametrize("use_float", [False, True], ids=["d", "f"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_binding_raises_value_error(use_float, case):
    row, col = BAD[case]
    with pytest.raises(ValueError, match="outside the matrix"):
        api.coo_to_csr_csc(V.Triplets(row, col, np.full(len(row), 1.5), (DIMA, DIMB)), use_float)
