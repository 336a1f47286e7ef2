"""CPU-side checks of the batched ranks among candidate lists shared between users (include/poismf_hip.h section 1k): the header
declares the three prototypes with the agreed parameter names, every library flavour exports them and the constants match
poismf_amd.api; the one scratch allocation of a call stays inside the budget for any arguments and never shrinks when an argument
grows; every invalid input answers 2 from the C entry point with nothing written (the checks run before any device work), and
raises from the Python wrappers; and calls without include_of still reach the entry points they reached before."""
import numpy as np
import pytest
import scipy.sparse as sp

from poismf_amd import api, build
from tests.test_rank_include_cpu import K, NITEMS, NUSERS, X_OK, _define, _fake_fitted, _NoDeviceSession, _params, _Recorder

NAMES = ("poismf_hip_rank_shared", "poismf_hip_session_rank_shared", "poismf_hip_rank_shared_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build()


# ---- 1. the boundary --------------------------------------------------------------------------------------------------------------

def test_header_declares_the_prototypes():
    ret, names = _params("poismf_hip_rank_shared")
    assert ret == "int"
    assert names == ["A", "B", "k", "dimA", "dimB", "users", "n_users", "test_indptr", "test_indices", "list_indptr", "list_indices",
                     "n_lists", "list_of", "unite_test", "excl_indptr", "excl_indices", "out_rank", "out_n_adm"]
    ret, names = _params("poismf_hip_session_rank_shared")
    assert ret == "int"
    assert names == ["s", "users", "n_users", "test_indptr", "test_indices", "list_indptr", "list_indices", "n_lists", "list_of",
                     "unite_test", "exclude_seen", "excl_indptr", "excl_indices", "out_rank", "out_n_adm"]
    ret, names = _params("poismf_hip_rank_shared_scratch_bytes")
    assert ret == "size_t" and names == ["n_users", "n_test_cells", "n_lists", "n_list_cells", "dimB", "k"]
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS
    assert _define("POISMF_HIP_RANK_SHARED_CHUNK_CELLS") == api.RANK_SHARED_CHUNK_CELLS >= api.RANK_BATCH_MAX_ROW
    assert _define("POISMF_HIP_TOPN_SHARED_MAX_CELLS") == api.TOPN_SHARED_MAX_CELLS


@pytest.mark.parametrize("use_float", [False, True, "r"])
def test_libraries_export_rank_shared(use_float):
    lib = api.load_library(use_float)
    for n in NAMES:
        assert getattr(lib, n) is not None


# ---- 2. the scratch ------------------------------------------------------------------------------------------------------------------

USERS = [1, 2, 63, 64, 65, 1000, 4096, 10 ** 5, 262144, 262145, 10 ** 6, 10 ** 7]
CELLS = [0, 1, 10, 65536, 524287, 524288, 524289, 10 ** 7, 10 ** 8]
TABLE = [0, 1, 100, 10 ** 4, 10 ** 6, 2 ** 24 - 1, 2 ** 24]
ITEMS = [1, 64, 3000, 10 ** 5, 2 ** 31 - 1]


@pytest.mark.parametrize("flavour", [False, True], ids=["d", "f"])
def test_scratch_stays_inside_the_budget_and_never_shrinks(flavour):
    """users 1 .. 10^7, held-out cells 0 .. 10^8, table 0 .. 2^24 indices, dimB 1 .. 2^31 - 1: at most 256 MiB, and no smaller
    when one argument grows with the others held"""
    budget = _define("POISMF_HIP_TOPN_BATCH_BUDGET_MB") << 20
    assert budget == 256 << 20
    fn = api.load_library(flavour).poismf_hip_rank_shared_scratch_bytes
    size = np.empty((len(USERS), len(CELLS), len(TABLE), len(ITEMS)), np.int64)
    for a, m in enumerate(USERS):
        for b, c in enumerate(CELLS):
            for d, n in enumerate(TABLE):
                for e, dimB in enumerate(ITEMS):
                    size[a, b, d, e] = int(fn(m, c, 1 + n // 1000, n, dimB, 50))
                    assert 0 < size[a, b, d, e] <= budget, (m, c, n, dimB, size[a, b, d, e])
    for axis in range(4):
        assert (np.diff(size, axis=axis) >= 0).all(), axis
    kmax = 512 if flavour else 256
    for k in (1, kmax):
        for g in (1, 10 ** 6):
            assert int(fn(4096, 40960, g, 10 ** 4, 10 ** 5, k)) == int(fn(4096, 40960, 1, 10 ** 4, 10 ** 5, 50))
    # a small call does not pay for a large one, and the bound is not vacuous
    assert int(fn(64, 640, 1, 1000, 3000, 50)) < (1 << 20)
    assert size.max() > (budget >> 1)


# ---- 3. invalid input ------------------------------------------------------------------------------------------------------------------

# (users, test, table, list_of, exclude), lists as (indptr, indices): every one invalid
OK_T, OK_L, OK_OF = ([0, 1, 2], [3, 4]), ([0, 2, 4], [3, 9, 4, 7]), [1, 0]
BAD = {
    "user-out-of-range": ([0, NUSERS], OK_T, OK_L, OK_OF, None),
    "negative-user": ([-1, 0], OK_T, OK_L, OK_OF, None),
    "test-item-out-of-range": ([0, 1], ([0, 1, 2], [3, NITEMS]), OK_L, OK_OF, None),
    "list-item-out-of-range": ([0, 1], OK_T, ([0, 2, 4], [3, 9, 4, NITEMS]), OK_OF, None),
    "list-negative-item": ([0, 1], OK_T, ([0, 2, 4], [-3, 9, 4, 7]), OK_OF, None),
    "exclude-item-out-of-range": ([0, 1], OK_T, OK_L, OK_OF, ([0, 1, 2], [3, NITEMS])),
    "list-unsorted-row": ([0, 1], OK_T, ([0, 2, 4], [9, 3, 4, 7]), OK_OF, None),
    "list-repeated-item": ([0, 1], OK_T, ([0, 2, 4], [3, 9, 7, 7]), OK_OF, None),
    "unreferenced-list-unsorted": ([0, 1], OK_T, ([0, 2, 4, 6], [3, 9, 4, 7, 8, 2]), OK_OF, None),
    "test-unsorted-row": ([0, 1], ([0, 2, 4], [1, 2, 9, 7]), OK_L, OK_OF, None),
    "exclude-unsorted-row": ([0, 1], OK_T, OK_L, OK_OF, ([0, 2, 4], [1, 2, 9, 7])),
    "list-decreasing-indptr": ([0, 1], OK_T, ([0, 2, 1], [3, 9]), OK_OF, None),
    "test-decreasing-indptr": ([0, 1], ([0, 2, 1], [1, 2]), OK_L, OK_OF, None),
    "exclude-decreasing-indptr": ([0, 1], OK_T, OK_L, OK_OF, ([0, 2, 1], [1, 2])),
    "list-of-out-of-range": ([0, 1], OK_T, OK_L, [0, 2], None),
    "list-of-negative": ([0, 1], OK_T, OK_L, [-1, 0], None),
    "list-of-wrong-length": ([0, 1], OK_T, OK_L, [0, 1, 1], None),
    "test-wrong-rows": ([0, 1], ([0, 1, 2, 3], [1, 2, 3]), OK_L, OK_OF, None),
}
NO_ROW_COUNT = {"list-of-wrong-length", "test-wrong-rows"}   # (a C caller has no row count to get wrong)


def _c_call(flavour, users, test, table, list_of, excl, unite=0, n_users=None, k=K, null=(), n_lists=None, dimB=NITEMS):
    """poismf_hip_rank_shared itself through ctypes; index arrays in the flavour's sparse_ix.  null: names of pointers passed as
    NULL.  Returns (rc, out_rank, out_n_adm), the outputs filled with marks beforehand."""
    lib = api.load_library(flavour)
    it = np.int32 if flavour == "r" else np.uint64
    dt = np.float32 if flavour is True else np.float64

    def ix(a):
        a = np.asarray(a, np.int64)
        return a.astype(it) if flavour == "r" else a.view(np.uint64).copy()

    A, B = np.ones((NUSERS, max(k, 1)), dt), np.ones((dimB, max(k, 1)), dt)
    u = ix(users)
    m = len(u) if n_users is None else n_users
    tp, ti, lp, li, lof = ix(test[0]), ix(test[1]), ix(table[0]), ix(table[1]), ix(list_of)
    G = len(lp) - 1 if n_lists is None else n_lists
    rank = np.full(max(len(ti), 1), 12345, np.uint32)
    n_adm = np.full(max(m, 1), 54321, np.uint32)
    p = api._ptr
    ep, ei = (ix(excl[0]), ix(excl[1])) if excl is not None else (None, None)
    rc = lib.poismf_hip_rank_shared(p(A), p(B), k, NUSERS, dimB, p(u), m, None if "test_indptr" in null else p(tp), p(ti),
                                    None if "list_indptr" in null else p(lp), p(li), G, None if "list_of" in null else p(lof), unite,
                                    p(ep) if ep is not None else None, p(ei) if ei is not None else None, p(rank), p(n_adm))
    return rc, rank, n_adm


def _untouched(rc, rank, n_adm, want=2):
    return rc == want and np.all(rank == 12345) and np.all(n_adm == 54321)


FLAVOURS = pytest.mark.parametrize("flavour", [False, True, "r"], ids=["d", "f", "r"])


@FLAVOURS
@pytest.mark.parametrize("unite", [0, 1])
@pytest.mark.parametrize("case", sorted(set(BAD) - NO_ROW_COUNT))
def test_c_entry_returns_2_and_writes_nothing(flavour, case, unite):
    users, test, table, list_of, excl = BAD[case]
    assert _untouched(*_c_call(flavour, users, test, table, list_of, excl, unite=unite))


@FLAVOURS
@pytest.mark.parametrize("which", ["test_indptr", "list_indptr", "list_of"])
def test_c_entry_null_pointers(flavour, which):
    assert _untouched(*_c_call(flavour, [0, 1], OK_T, OK_L, OK_OF, None, null=(which,)))


@FLAVOURS
def test_c_entry_no_lists_with_users_present(flavour):
    assert _untouched(*_c_call(flavour, [0, 1], OK_T, ([0], []), [0, 0], None, n_lists=0))


@FLAVOURS
def test_c_entry_no_users_is_not_an_error(flavour):
    assert _untouched(*_c_call(flavour, [0], ([0, 1], [3]), ([0, 1], [3]), [0], None, n_users=0), want=0)
    assert _untouched(*_c_call(flavour, [0], ([0, 1], [3]), ([0], []), [0], None, n_users=0, n_lists=0), want=0)


@pytest.mark.parametrize("flavour,kmax", [(False, 256), (True, 512), ("r", 256)], ids=["d", "f", "r"])
def test_c_entry_k_out_of_range(flavour, kmax):
    for k in (0, -1, kmax + 1):
        assert _untouched(*_c_call(flavour, [0, 1], OK_T, OK_L, OK_OF, None, k=k))


@FLAVOURS
def test_c_entry_overlong_rows(flavour):
    """a held-out row one cell over POISMF_HIP_RANK_BATCH_MAX_ROW; an exclusion row longer than the catalogue (which section 1f's
    limit bounds from above for any dimB below it); a table one index over POISMF_HIP_TOPN_SHARED_MAX_CELLS, refused by its row
    pointers before an index is read"""
    n = api.RANK_BATCH_MAX_ROW + 1
    row = np.arange(n)
    assert _untouched(*_c_call(flavour, [0], ([0, n], row), ([0, 2], [3, 9]), [0], None, k=1, dimB=n))
    rc, rank, n_adm = _c_call(flavour, [0], ([0, n - 1], row[:-1]), ([0, 2], [3, 9]), [0], ([0, n + 1], np.arange(n + 1)), k=1, dimB=n)
    assert rc == 2 and np.all(rank == 12345) and np.all(n_adm == 54321)
    big = api.TOPN_SHARED_MAX_CELLS + 1
    assert _untouched(*_c_call(flavour, [0], ([0, 1], [3]), ([0, big // 2, big], [3, 9]), [0], None, k=1))


@pytest.mark.parametrize("case", sorted(BAD))
def test_python_wrappers_raise_before_the_device(case):
    users, test, table, list_of, excl = BAD[case]
    for unite in (False, True):
        with pytest.raises(ValueError):
            _NoDeviceSession(True).rank_batch(users, test, exclude=excl, include=table, include_of=list_of, unite_test=unite)
        for dt in (np.float32, np.float64):
            with pytest.raises(ValueError):
                api.rank_batch(np.ones((NUSERS, K), dt), np.ones((NITEMS, K), dt), users, test, exclude=excl, include=table,
                               include_of=list_of, unite_test=unite)


def _both(**kw):
    """the two Python entry points, neither near a device"""
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    return (lambda: _NoDeviceSession(True).rank_batch([0, 1], OK_T, **kw)), (lambda: api.rank_batch(A, B, [0, 1], OK_T, **kw))


@pytest.mark.parametrize("kw,match", [
    (dict(include_of=[0, 1]), "needs include"),                                       # include_of without include
    (dict(include=OK_L, include_of=[0]), "entries for 2 users"),                      # wrong length
    (dict(include=OK_L, include_of=[0, 2]), "not a row"),                             # an entry >= G
    (dict(include=OK_L, include_of=True), "integers"),                                # bool
    (dict(include=OK_L, include_of=-1), "negative"),
    (dict(include=OK_L, include_of=[[0, 1]]), "1-d"),
    (dict(include=([0, 2, 4], [9, 3, 4, 7]), include_of=0), "ascending"),             # an unsorted table row
    (dict(include=([0], []), include_of=0), "no rows"),
    (dict(include=OK_L, unite_test=True), "unite_test needs include_of"),            # unite_test without include_of
    (dict(unite_test=True), "unite_test needs include_of"),
], ids=["no-include", "wrong-length", "entry-over-G", "bool", "negative-int", "two-d", "unsorted-table", "empty-table", "unite-alone",
        "unite-bare"])
def test_python_argument_errors(kw, match):
    for call in _both(**kw):
        with pytest.raises(ValueError, match=match):
            call()


def test_python_overlong_rows():
    """a held-out row over 65 536 cells, and a table over the cell limit (two rows of 2^23 + 1 indices: built once)"""
    n = api.RANK_BATCH_MAX_ROW + 1
    row = np.arange(n)
    B = np.ones((n, 2), np.float32)
    for unite in (False, True):
        with pytest.raises(ValueError, match="longer"):
            api.rank_batch(np.ones((2, 2), np.float32), B, [0], ([0, n], row), include=([0, 2], [3, 9]), include_of=0, unite_test=unite)
    half = api.TOPN_SHARED_MAX_CELLS // 2 + 1
    table = (np.array([0, half, 2 * half], np.uint64), np.tile(np.arange(half, dtype=np.uint64), 2))
    assert len(table[1]) > api.TOPN_SHARED_MAX_CELLS
    s = _NoDeviceSession(True)
    s.dimB = half
    with pytest.raises(ValueError, match="more than"):
        s.rank_batch([0], ([0, 1], [3]), include=table, include_of=0)


def test_session_exclude_seen_outside_the_shard():
    with pytest.raises(ValueError, match="outside"):
        _NoDeviceSession(True).rank_batch([1, 5], OK_T, exclude_seen=True, include=OK_L, include_of=OK_OF)   # (user 5: rows 0..3)


BAD_EVAL = {
    "no-include": (None, 0),
    "table-too-wide": (sp.csr_matrix((2, NITEMS + 1)), 0),
    "of-wrong-length": (OK_L, [0] * (NUSERS - 1)),
    "of-entry-over-G": (OK_L, [0, 2, 0, 0, 0, 0]),
    "of-bool": (OK_L, True),
    "of-two-d": (OK_L, [[0] * NUSERS]),
    "table-unsorted": (([0, 2, 4], [9, 3, 4, 7]), 0),
}


@pytest.mark.parametrize("case", sorted(BAD_EVAL))
def test_eval_ranking_raises_before_the_device(case):
    table, of = BAD_EVAL[case]
    for use_float in (False, True):
        with pytest.raises(ValueError):
            _fake_fitted(use_float).eval_ranking(X_OK, include=table, include_of=of)
    with pytest.raises(ValueError):
        _NoDeviceSession(True).eval_ranking(X_OK, include=table, include_of=of, exclude_seen=False)


# ---- 4. what reaches the library ---------------------------------------------------------------------------------------------------

def test_include_of_selects_the_entry_point(monkeypatch):
    """without include_of the wrappers reach the entry points of sections 1g and 1j with the arguments they had; with it, section
    1k's"""
    rec = _Recorder()
    s = _NoDeviceSession(True, rec)
    s.rank_batch([0, 1], OK_T)
    s.rank_batch([0, 1], OK_T, include=OK_L)
    s.rank_batch([0, 1], OK_T, include=OK_L, include_of=OK_OF)
    s.rank_batch([0, 1], OK_T, include=OK_L, include_of=1, unite_test=True)
    s.eval_ranking(X_OK, exclude_seen=False, include=OK_L, include_of=0)
    assert rec.calls == [("poismf_hip_session_rank_batch", 10), ("poismf_hip_session_rank_include", 12)] + [("poismf_hip_session_rank_shared", 15)] * 3
    rec = _Recorder()
    monkeypatch.setattr(api, "load_library", lambda use_float: rec)
    A, B = np.ones((NUSERS, K), np.float32), np.ones((NITEMS, K), np.float32)
    api.rank_batch(A, B, [0, 1], OK_T)
    api.rank_batch(A, B, [0, 1], OK_T, include=OK_L)
    api.rank_batch(A, B, [0, 1], OK_T, include=OK_L, include_of=OK_OF)
    _fake_fitted(True).eval_ranking(X_OK, include=OK_L, include_of=[1, 0, 0, 0, 0, 1])
    assert rec.calls == [("poismf_hip_rank_batch", 13), ("poismf_hip_rank_include", 15), ("poismf_hip_rank_shared", 18),
                         ("poismf_hip_rank_shared", 18)]


def test_eval_ranking_passes_the_pool_as_it_is(monkeypatch):
    """what reaches rank_batch: the table untouched, the entries of include_of for the evaluated users, the united mode"""
    seen = {}

    def fake(A, B, users, test, exclude=None, include=None, include_of=None, unite_test=False):
        seen.update(include=include, include_of=include_of, unite_test=unite_test, users=users)
        return np.zeros(len(test[1]), np.uint32), np.ones(len(users), np.uint32)

    monkeypatch.setattr(api, "rank_batch", fake)
    _fake_fitted(True).eval_ranking(X_OK, include=OK_L, include_of=[1, 0, 1, 1, 1, 1])      # users default to rows 0 and 1 of X_OK
    assert seen["include"] is OK_L and seen["unite_test"] is True
    assert seen["users"].tolist() == [0, 1] and np.asarray(seen["include_of"]).tolist() == [1, 0]
    _fake_fitted(True).eval_ranking(X_OK, include=OK_L, include_of=[1, 0, 1, 1, 1, 0], users=[5, 1])
    assert np.asarray(seen["include_of"]).tolist() == [0, 0]
    _fake_fitted(True).eval_ranking(X_OK, include=OK_L, include_of=1)
    assert seen["include_of"] == 1
