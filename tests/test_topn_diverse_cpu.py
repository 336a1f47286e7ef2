"""CPU-side checks of the diversified batched top-N (include/poismf_hip.h section 1p): the header's defines equal the api constants,
the three symbols are declared with the agreed parameter names, exported by every flavour and built from a unit of their own; the C
entry point answers 2 / 0 without a device on the malformed cases; the Python checks raise on the same cases before any library call;
the one scratch allocation stays inside the budget and never shrinks when the batch grows; and the reference the GPU tests compare
against gives hand-written answers."""
import numpy as np
import pytest

from poismf_amd import api, build
from tests.test_gpu_topn_diverse import diverse_expect
from tests.test_topn_batch_cpu import BAD as BAD_BATCH, NITEMS, NUSERS, K, _NoDeviceSession, _define, _fake_fitted, _params

NAMES = ("poismf_hip_topn_diverse", "poismf_hip_session_topn_diverse", "poismf_hip_topn_diverse_scratch_bytes")
ONES = [1.0] * NITEMS

# section 1f's table; what is left after exclusion no longer matters, and the limit on n is 1f's
BAD = {c: v for c, v in BAD_BATCH.items() if c != "n-above-items-left"}
# (n, pool, lam, inverse norms): every one invalid
BAD_OWN = {
    "n-above-128": (129, 200, 0.5, ONES),
    "pool-below-n": (5, 4, 0.5, ONES),
    "pool-above-1024": (5, 1025, 0.5, ONES),
    "lam-nan": (5, 20, float("nan"), ONES),
    "lam-negative": (5, 20, -1e-9, ONES),
    "lam-above-one": (5, 20, 1.0000001, ONES),
    "inv-null": (5, 20, 0.5, None),
    "inv-nan": (5, 20, 0.5, ONES[:-1] + [float("nan")]),
    "inv-inf": (5, 20, 0.5, [float("inf")] + ONES[1:]),
    "inv-negative": (5, 20, 0.5, ONES[:7] + [-1e-30] + ONES[8:]),
}


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


def test_header_declares_the_prototypes_and_the_constants_agree():
    assert _params("poismf_hip_topn_diverse") == ("int", ["A", "B", "k", "dimA", "dimB", "users", "n_users", "n_top", "pool", "lambda",
                                                          "item_inv_norm", "excl_indptr", "excl_indices", "out_ix", "out_score", "out_value"])
    assert _params("poismf_hip_session_topn_diverse") == ("int", ["s", "users", "n_users", "n_top", "pool", "lambda", "item_inv_norm",
                                                                  "exclude_seen", "excl_indptr", "excl_indices", "out_ix", "out_score",
                                                                  "out_value"])
    assert _params("poismf_hip_topn_diverse_scratch_bytes") == ("size_t", ["n_users", "n_top", "pool", "dimB", "k"])
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert build.UNITS["topn_diverse"] == ("topn_diverse.hip", [])
    assert {"tb_deep.hpp", "tb_gather.hpp", "wave_ops.hpp"} <= set(build._deps("topn_diverse.hip"))
    assert _define("POISMF_HIP_TOPN_DIVERSE_MAX_ITEMS") == api.TOPN_DIVERSE_MAX_ITEMS == 2 ** 24
    # the budget: section 1l's, and the inverse norms at their largest (8 B x 2^24 items)
    assert _define("POISMF_HIP_TOPN_DIVERSE_BUDGET_MB") == api.TOPN_DIVERSE_BUDGET_MB == _define("POISMF_HIP_TOPN_DEEP_BUDGET_MB") + 128


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_topn_diverse(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


def _c_call(flavour, users, n, excl, pool=20, lam=0.5, inv=ONES, n_users=None, dimB=NITEMS):
    """poismf_hip_topn_diverse itself through ctypes; index arrays in the flavour's sparse_ix, the norms in its real_t"""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    shape = (max(m, 1), max(n, 1))
    out, sc, val = np.full(shape, 12345, it), np.full(shape, -7.0, dt), np.full(shape, -7.0, dt)
    p = api._ptr
    ip, ii = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    w = np.asarray(inv, dt) if inv is not None else None
    rc = lib.poismf_hip_topn_diverse(p(A), p(B), K, NUSERS, dimB, p(u), m, n, pool, lam, p(w) if w is not None else None,
                                     p(ip) if ip is not None else None, p(ii) if ii is not None else None, p(out), p(sc), p(val))
    return rc, out, sc, val


def _untouched(out, sc, val):
    return np.all(out == 12345) and np.all(sc == -7.0) and np.all(val == -7.0)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(set(BAD) - {"exclude-wrong-rows"}))   # (a C caller has no row count to get wrong)
def test_c_entry_returns_2_on_section_1l_s_cases(flavour, case):
    users, n, excl = BAD[case]
    rc, *outs = _c_call(flavour, users, n, excl, pool=max(n, 20))
    assert rc == 2 and _untouched(*outs)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
@pytest.mark.parametrize("case", sorted(BAD_OWN))
def test_c_entry_returns_2_on_its_own_cases(flavour, case):
    n, pool, lam, inv = BAD_OWN[case]
    rc, *outs = _c_call(flavour, [0, 1], n, None, pool=pool, lam=lam, inv=inv)
    assert rc == 2 and _untouched(*outs)


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_too_many_items_and_no_users(flavour):
    """dimB = 2^24 + 1 is refused before the norms are read (the arrays here are far shorter); no users: 0 whatever else is passed"""
    rc, *outs = _c_call(flavour, [0, 1], 5, None, dimB=2 ** 24 + 1)
    assert rc == 2 and _untouched(*outs)
    rc, *outs = _c_call(flavour, [0], 5, None, n_users=0)
    assert rc == 0 and _untouched(*outs)
    rc, *outs = _c_call(flavour, [0], 0, None, pool=0, lam=7.0, inv=None, n_users=0)
    assert rc == 0


def test_c_entry_k_out_of_range():
    lib = api.load_library(True)
    A = np.ones((2, 4), np.float32)
    u, w, out = np.zeros(1, np.uint64), np.ones(2, np.float32), np.zeros(1, np.uint64)
    p = api._ptr
    for k in (0, -1, 513):
        assert lib.poismf_hip_topn_diverse(p(A), p(A), k, 2, 2, p(u), 1, 1, 1, 0.5, p(w), None, None, p(out), None, None) == 2


@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_c_entry_the_ends_of_the_ranges_are_not_an_argument_error(flavour):
    """past the checks the call needs a device: 0 where there is one, 1 where there is none, never 2.  A pool above the number of items
    and a row with nothing left are short rows, not errors"""
    for n, pool, lam in ((1, 1, 0.0), (128, 128, 1.0), (128, 1024, 0.5), (5, 1024, 1.0)):
        assert _c_call(flavour, [0, 1], n, None, pool=pool, lam=lam)[0] in (0, 1)
    assert _c_call(flavour, [0, 1], 5, ([0, 0, NITEMS], list(range(NITEMS))))[0] in (0, 1)
    assert _c_call(flavour, [0, 1], 5, None, inv=[0.0] * (NITEMS - 1) + [-0.0])[0] in (0, 1)


# ---- Python ----
def test_the_call_needs_a_fitted_model():
    with pytest.raises(ValueError, match="not been fitted"):
        api.PoisMF(k=3).topN_diverse([0, 1])


@pytest.mark.parametrize("use_float", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_input_raises_before_the_device(use_float, case):
    """(no item_norm: the norms would be computed on a device, after the checks)"""
    users, n, excl = BAD[case]
    with pytest.raises(ValueError):
        _fake_fitted(use_float).topN_diverse(users, n, pool=max(n, 20), exclude=excl)
    with pytest.raises(ValueError):
        _NoDeviceSession(use_float).topn_diverse(users, n, pool=max(n, 20), exclude=excl)


PY_MESSAGES = {"n-above-128": "above the batched limit", "pool-below-n": "below n", "pool-above-1024": "above the deep batched limit",
               "lam-nan": r"outside \[0, 1\]", "lam-negative": r"outside \[0, 1\]", "lam-above-one": r"outside \[0, 1\]",
               "inv-null": "required", "inv-nan": "NaN", "inv-inf": "infinite", "inv-negative": "negative"}


@pytest.mark.parametrize("case", sorted(BAD_OWN))
def test_the_argument_helper_rejects_what_returns_2(case):
    n, pool, lam, inv = BAD_OWN[case]
    with pytest.raises(ValueError, match=PY_MESSAGES[case]):
        api._topn_diverse_args([0, 1], n, pool, lam, inv, None, NUSERS, NITEMS, np.float32)
    if not case.startswith("inv-"):
        with pytest.raises(ValueError, match=PY_MESSAGES[case]):
            _fake_fitted(True).topN_diverse([0, 1], n, pool, lam)
        with pytest.raises(ValueError, match=PY_MESSAGES[case]):
            _NoDeviceSession(True).topn_diverse([0, 1], n, pool, lam)


def test_the_argument_helper_on_the_rest():
    for lam in ("0.5", None, True, [0.5]):
        with pytest.raises(ValueError, match="real number"):
            api._topn_diverse_args([0, 1], 5, 20, lam, ONES, None, NUSERS, NITEMS)
    with pytest.raises(ValueError, match="must be positive"):
        api._topn_diverse_args([0, 1], 0, 20, 0.5, ONES, None, NUSERS, NITEMS)
    with pytest.raises(ValueError, match=f"{NITEMS - 1} inverse norms for {NITEMS} items"):
        api._topn_diverse_args([0, 1], 5, 20, 0.5, ONES[:-1], None, NUSERS, NITEMS)
    with pytest.raises(ValueError, match="limit of 16777216"):
        api._topn_diverse_args([0, 1], 5, 20, 0.5, ONES, None, NUSERS, 2 ** 24 + 1)
    with pytest.raises(ValueError, match="infinite in the model's precision"):       # (judged after the conversion)
        api._topn_diverse_args([0], 5, 20, 0.5, ONES[:-1] + [1e39], None, NUSERS, NITEMS, np.float32)
    u, inv, indptr, indices = api._topn_diverse_args([1, 0, 1], 5, 5, 1, np.arange(NITEMS), ([0, 1, 1, 3], [4, 2, 9]), NUSERS, NITEMS, np.float32)
    assert u.dtype == np.uint64 and u.tolist() == [1, 0, 1] and inv.dtype == np.float32 and inv.flags.c_contiguous
    assert indptr.tolist() == [0, 1, 1, 3] and indices.tolist() == [4, 2, 9]
    assert api._topn_diverse_args([], 128, 1024, 0.0, ONES, None, NUSERS, NITEMS)[2] is None
    # item_norm= takes squared norms, as similar_items does, and is judged as there
    with pytest.raises(ValueError, match="finite and non-negative"):
        _fake_fitted(True).topN_diverse([0, 1], 5, item_norm=ONES[:-1] + [-1.0])
    with pytest.raises(ValueError, match="entries for"):
        _NoDeviceSession(True).topn_diverse([0, 1], 5, item_norm=ONES[:-1])
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).topn_diverse([1, 5], 5, exclude_seen=True, item_norm=ONES)
    ix, sc, val = _fake_fitted(True).topN_diverse([], 7, output_score=True)
    assert ix.shape == (0, 7) and sc.shape == (0, 7) and val.shape == (0, 7) and sc.dtype == np.float32
    with pytest.raises(AttributeError):                               # (past the checks: the library is next)
        _NoDeviceSession(True).topn_diverse([1, 2], 5, item_norm=ONES)


# ---- scratch ----
@pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])
def test_scratch_stays_inside_the_budget(flavour):
    budget = _define("POISMF_HIP_TOPN_DIVERSE_BUDGET_MB") << 20
    lib = api.load_library(flavour)
    fn, deep = lib.poismf_hip_topn_diverse_scratch_bytes, lib.poismf_hip_topn_deep_scratch_bytes
    real = 4 if flavour is True else 8
    batch = sorted({1, 2, 63, 64, 65, 1000, 4096, 10 ** 5, 10 ** 6, 10 ** 7} | {int(x) for x in np.logspace(0, 7, 30)})
    size = {}
    for n, pool in ((1, 1), (10, 100), (10, 1024), (128, 128), (128, 1024)):
        for dimB in (1, 40, 10 ** 5, 2 ** 24):
            for m in batch:
                b = size[n, pool, dimB, m] = int(fn(m, n, pool, dimB, 50))
                assert 0 < b <= budget, (m, n, pool, dimB, b)
                assert b >= real * dimB + n * min(m, 64) * (4 + 2 * real)             # the norms and the picked rows of a tile of users
                assert b - real * dimB <= _define("POISMF_HIP_TOPN_DEEP_BUDGET_MB") << 20   # all but the norms: section 1l's budget
                for k in (1, 512):
                    assert int(fn(m, n, pool, dimB, k)) == b                          # no part depends on k
            later = [size[n, pool, dimB, m] for m in batch]
            assert later == sorted(later), (n, pool, dimB)                            # it never shrinks when the batch grows
            assert later[-1] == later[-2]                                             # ... and stops growing: the chunk is full
    assert int(fn(64, 10, 100, 1000, 50)) < (16 << 20)                                # a small call does not pay for a large one
    assert max(size.values()) > (budget >> 1)                                         # (the bound is not vacuous)
    # the deep call's own sizes are what they were: the layout moved to a header, with nothing added for a caller that adds nothing
    assert int(deep(1, 1024, 10 ** 6, 50)) == (16595264 if real == 8 else 12396864)
    assert int(deep(10 ** 7, 1024, 10 ** 6, 50)) == (1073246240 if real == 8 else 1073348128)


# ---- the reference of tests/test_gpu_topn_diverse.py ----
def _answer(A, B, excl, n, pool, lam, dt=np.float32):
    """on small integers every chain is exact, so plain products stand in for the fused chain"""
    A, B = np.asarray(A, dt), np.asarray(B, dt)
    rel = (A @ B.T).astype(dt)
    n2 = (B * B).sum(axis=1)
    inv = np.zeros(len(B), dt)
    inv[n2 != 0] = dt(1) / np.sqrt(n2[n2 != 0].astype(dt))
    ix, sc, val = diverse_expect(rel, lambda P: (B[P] @ B[P].T).astype(dt), inv, excl, n, pool, lam)
    return ix[0].tolist(), sc[0].tolist(), val[0].tolist()


def test_reference_on_hand_written_cases():
    NONE, ninf = api.TOPN_NONE, -np.inf
    # three items, items 0 and 1 identical, item 2 orthogonal to them and a little less relevant: relevances 10, 10, 8
    A, B = [[10.0, 8.0]], [[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    none = [[]]
    f = np.float32
    # lam = 1: the plain order, the duplicate second; values r = 1, 1, 0.8
    assert _answer(A, B, none, 3, 3, 1.0) == ([0, 1, 2], [10.0, 10.0, 8.0], [1.0, 1.0, float(f(8) / f(10))])
    # lam < 1: once item 0 is picked its copy carries the whole penalty and comes last
    for lam in (0.7, 0.3):
        lam_t, oml = f(lam), f(1.0 - lam)
        second = lam_t * (f(8) / f(10)) - oml * f(0)
        third = lam_t * f(1) - oml * f(1)
        assert float(third) < float(second)
        assert _answer(A, B, none, 3, 3, lam) == ([0, 2, 1], [10.0, 8.0, 10.0], [float(lam_t * f(1)), float(second), float(third)])
    # lam = 0: relevance plays no part; every value before a pick is 0 and ties go to the lowest position, then the orthogonal item
    assert _answer(A, B, none, 3, 3, 0.0) == ([0, 2, 1], [10.0, 8.0, 10.0], [0.0, 0.0, -1.0])
    # the pool bounds the picks: pool = 2 never sees item 2; n = 2 of pool 3 stops after the orthogonal item
    assert _answer(A, B, none, 3, 2, 0.7)[0] == [0, 1, NONE]
    assert _answer(A, B, none, 2, 3, 0.7)[0] == [0, 2]
    # exclusions shape the pool; a short row is padded in all three outputs; nothing left: all padding
    assert _answer(A, B, [[0]], 3, 3, 0.7) == ([1, 2, NONE], [10.0, 8.0, ninf], [float(f(0.7) * f(1)), float(f(0.7) * (f(8) / f(10))), ninf])
    assert _answer(A, B, [[0, 1, 2]], 2, 3, 0.7) == ([NONE, NONE], [ninf, ninf], [ninf, ninf])
    # a zero row has cosine 0 to everything: never penalised; rel_0 <= 0 leaves the relevances undivided
    assert _answer([[1.0, 1.0]], [[2.0, 0.0], [2.0, 0.0], [0.0, 0.0]], none, 3, 3, 0.3)[0] == [0, 2, 1]
    # ... and at lam = 0.5 the copy's 0.5 - 0.5 ties with the zero row's 0 - 0: the lower position wins
    assert _answer([[1.0, 1.0]], [[2.0, 0.0], [2.0, 0.0], [0.0, 0.0]], none, 3, 3, 0.5)[0] == [0, 1, 2]
    ix, sc, val = _answer([[-1.0, -2.0]], [[1.0, 0.0], [0.0, 1.0]], none, 2, 2, 1.0)
    assert (ix, sc, val) == ([0, 1], [-1.0, -2.0], [-1.0, -2.0])
    # the arithmetic is the rows': in float32 0.7 x 0.8 - 0.3 x 0 is not the double's value
    assert _answer(A, B, none, 3, 3, 0.7)[2][1] != 0.7 * 0.8
    assert _answer(A, B, none, 3, 3, 0.7, np.float64)[2][1] == 0.7 * (8.0 / 10.0) - (1.0 - 0.7) * 0.0


def test_the_gpu_test_s_inputs_make_mmr_bite():
    """what tests/test_gpu_topn_diverse.py asserts about its inputs at lam = 0.7, checked here with host products in place of the
    chains (a rounding apart, which moves no tenth of the rows): MMR changes at least a tenth of the rows' top 10, at every k"""
    from tests import test_gpu_topn_diverse as G
    users = G.batch_users().astype(np.int64)
    for prec in (False, True):
        for k in G.KS:
            A, B = G.make_factors(k, prec)
            dt = B.dtype.type
            assert np.array_equal(B[350:450], B[0:100]) and not B[list(G.ZERO_ROWS)].any() and (B.any(axis=1).sum() == G.DIMB - 2)
            rel = (A[users] @ B.T).astype(dt)
            n2 = (B * B).sum(axis=1)
            inv = np.zeros(G.DIMB, dt)
            inv[n2 != 0] = dt(1) / np.sqrt(n2[n2 != 0])
            gram = (B @ B.T).astype(dt)
            got = diverse_expect(rel, lambda P: gram[np.ix_(P, P)], inv, [[]] * len(users), 10, 100, 0.7)[0]
            plain = diverse_expect(rel, lambda P: gram[np.ix_(P, P)], inv, [[]] * len(users), 10, 100, 1.0)[0]
            differ = int((got != plain).any(axis=1).sum())
            assert 10 * differ >= 3 * len(users), (k, prec, differ)      # (three tenths here: a margin over the GPU test's one)
