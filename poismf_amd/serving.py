"""The serving calls' host side: the argument checks that need no device, each rule written once, and the one path every batched
top-N and rank call takes to the library (include/poismf_hip.h sections 1f-1r).

A call is made against a *target*: a ``Session`` (resident factors) or ``api._HostFactors`` (host factors that go up with the call).
Both offer ``dimA``, ``dimB``, ``k``, ``use_float``, ``item_norms()`` and ``_entry(name, exclude_seen)``, which gives the library's
function for ``name``, its leading arguments and what stands in front of the exclusion lists: ``(A, B, k, dimA, dimB)`` and nothing
on host factors, the handle and the ``exclude_seen`` flag on a session.  Nothing here falls back to the CPU.

The limits these checks enforce are ``api``'s constants, read through ``api`` when a check runs.
"""
import ctypes as C

import numpy as np


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _opt_ptr(a):
    return _ptr(a) if a is not None and len(a) else None


def _real_t(use_float):
    return np.float32 if use_float else np.float64


def _batch_rc(rc, what):
    if rc == 2:
        raise ValueError(f"invalid arguments for the batched {what} (an index out of range, an unsorted or overlong row, or too few items left)")
    if rc:
        raise MemoryError(f"batched {what} failed (no usable HIP device or out of memory)")


# ---- the rules the calls share ------------------------------------------------------------------------------------------------------

def _index_array(a, what):
    """a 1-d index list as C-contiguous uint64; ValueError for a negative or non-integer entry"""
    a = np.asarray(a)
    if a.ndim != 1:
        a = a.reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers")
    if a.size and a.dtype.kind == "i" and int(a.min()) < 0:
        raise ValueError(f"{what}: negative index")
    return np.ascontiguousarray(a, dtype=np.uint64)


def _csr_list(lst, m, dimB, what, row_max=None, dense_ok=False, keep_zeros=False):
    """A per-user item list of the batched entry points -- a SciPy sparse matrix with one row per user (its stored columns,
    duplicates merged; cells stored as zero dropped unless keep_zeros), with dense_ok anything scipy.sparse.csr_matrix() accepts,
    or an (indptr, indices) pair -- checked as the library checks it: m rows, indices below dimB and strictly ascending within a
    row.  Returns (indptr, indices) as uint64 arrays starting at 0."""
    if isinstance(lst, (tuple, list)) and len(lst) == 2 and not hasattr(lst, "tocsr"):
        indptr, indices = _index_array(lst[0], what + " indptr"), _index_array(lst[1], what + " indices")
    else:
        import scipy.sparse as sp
        if not dense_ok and not sp.issparse(lst):
            raise ValueError(f"{what} must be a SciPy sparse matrix or an (indptr, indices) pair")
        csr = sp.csr_matrix(lst)
        if csr.shape[0] != m:
            raise ValueError(f"{what} has {csr.shape[0]} rows for {m} users")
        if csr.shape[1] > dimB:
            raise ValueError(f"{what} has more columns than there are items")
        csr.sum_duplicates()
        if not keep_zeros:
            csr.eliminate_zeros()
        csr.sort_indices()
        indptr, indices = _index_array(csr.indptr, what + " indptr"), _index_array(csr.indices, what + " indices")
    if len(indptr) != m + 1:
        raise ValueError(f"{what} has {max(len(indptr) - 1, 0)} rows for {m} users")
    if np.any(indptr[1:] < indptr[:-1]) or int(indptr[-1]) > len(indices):
        raise ValueError(f"{what}: row pointers must not decrease and must stay inside the index list")
    lo, hi = int(indptr[0]), int(indptr[-1])
    seg = indices[lo:hi]
    if len(seg) and int(seg.max()) >= dimB:
        raise ValueError(f"an item index of {what} is out of range")
    if len(seg) > 1:
        bad = seg[1:] <= seg[:-1]
        starts = indptr[1:-1].astype(np.int64) - lo - 1          # position (in bad) of each later row's first entry
        starts = starts[(starts >= 0) & (starts < len(bad))]
        bad[starts] = False
        if np.any(bad):
            raise ValueError(f"{what}: the item indices of a row must be strictly ascending")
    if row_max is not None and m and int((indptr[1:] - indptr[:-1]).max()) > row_max:
        raise ValueError(f"{what}: a row is longer than {row_max}")
    return np.ascontiguousarray(indptr - indptr[0]), np.ascontiguousarray(seg)


def _top_n(n, limit, which):
    """n as an int: positive and at most `limit`, the `which` ("batched" / "deep batched") limit of the message"""
    n = int(n)
    if n <= 0:
        raise ValueError("n must be positive")
    if n > limit:
        raise ValueError(f"n = {n} is above the {which} limit of {limit}")
    return n


def _users_and_n(users, n, limit, which, what="users"):
    """what every top-N check starts with: (users as uint64, n as an int within the limit); _users_in_range follows the rules on
    the number of items"""
    return _index_array(users, what), _top_n(n, limit, which)


def _users_in_range(users, dimA):
    if len(users) and int(users.max()) >= dimA:
        raise ValueError("a user index is out of range")


def _item_count(dimB, limit=None, call=None, empty_ok=False):
    """the rules on the number of items that differ per call: at least one, and at most the limit of `call`, the call's own word"""
    if dimB < 1 and not empty_ok:
        raise ValueError("there are no items")
    if limit is not None and dimB > limit:
        raise ValueError(f"{dimB} items are above the {call}'s limit of {limit}")


def _exclude_list(exclude, m, dimB):
    """the `exclude` of the top-N calls: (None, None), or its (indptr, indices) as uint64 arrays, stored zeros kept"""
    if exclude is None:
        return None, None
    return _csr_list(exclude, m, dimB, "exclude", dense_ok=True, keep_zeros=True)


def _finite_nonneg(a, dtype, nan, inf, neg):
    """`a` as a C-contiguous array of `dtype`, the model's real_t, finite and non-negative AFTER that conversion (a double above
    float32's range is refused for a float32 model).  The caller words the refusals: `nan` and `neg` whole, `inf` up to its verb."""
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(a, dtype=dtype)
    if np.isnan(a).any():
        raise ValueError(nan)
    if np.isinf(a).any():
        raise ValueError(f"{inf} infinite in the model's precision")
    if (a < 0).any():
        raise ValueError(neg)
    return a


def _topn_outputs(m, n, dt, output_score):
    """the output arrays of a top-N call: items and scores, the latter empty unless asked for"""
    return np.empty((m, n), np.uint64), np.empty((m, n) if output_score else (0, n), dt)


def _diverse_outputs(m, n, dt, output_score, output_value):
    """the three output arrays of the diversified calls: items, relevances and values, the latter two empty unless asked for"""
    return _topn_outputs(m, n, dt, output_score) + (np.empty((m, n) if output_value else (0, n), dt),)


def _outside_shard(users, shardA):
    """exclude_seen of a session's batched calls: its CSR holds the rows shardA of A only"""
    if len(users) and (int(users.min()) < shardA[0] or int(users.max()) >= shardA[1]):
        raise ValueError("exclude_seen: a user lies outside this session's rows of A")


# ---- the argument checks of each call -----------------------------------------------------------------------------------------------

def _topn_batch_args(users, n, exclude, dimA, dimB):
    """The argument checks of the batched top-N (include/poismf_hip.h section 1f) that need no device, as the library itself
    makes them; returns (users, excl_indptr or None, excl_indices or None) as uint64 arrays."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    m = len(users)
    if n > dimB:
        raise ValueError("n is larger than the number of items")
    _users_in_range(users, dimA)
    indptr, indices = _exclude_list(exclude, m, dimB)
    if indptr is not None and m and int((indptr[1:] - indptr[:-1]).max()) > dimB - n:
        raise ValueError("n is larger than the number of items a user has left after exclusion")
    return users, indptr, indices


def _new_rows_args(X_new, dimB, use_float):
    """The rows of users the model has never seen, as the fold-in calls take them (include/poismf_hip.h section 1m), checked without
    a device as the library itself checks them: a SciPy sparse matrix with one row per new user and the model's number of columns,
    coerced as transform() coerces it (CSR, duplicates summed, indices sorted).  Returns (data real_t, indptr, indices) with uint64
    index arrays."""
    import scipy.sparse as sp
    if not sp.issparse(X_new):
        raise ValueError("the new rows must be a SciPy sparse matrix with one row per new user")
    if X_new.shape[1] != dimB:
        raise ValueError(f"the new rows have {X_new.shape[1]} columns, the model {dimB} items")
    csr = sp.csr_matrix(X_new)
    if len(csr.indptr) != csr.shape[0] + 1 or np.any(np.diff(csr.indptr) < 0) or int(csr.indptr[-1]) > len(csr.indices):
        raise ValueError("the new rows: row pointers must not decrease and must stay inside the index list")
    if len(csr.indices) and (int(csr.indices.min()) < 0 or int(csr.indices.max()) >= dimB):
        raise ValueError("an item index of the new rows is out of range")
    csr.sum_duplicates(); csr.sort_indices()
    return (np.ascontiguousarray(csr.data, dtype=_real_t(use_float)), np.ascontiguousarray(csr.indptr, dtype=np.uint64),
            np.ascontiguousarray(csr.indices, dtype=np.uint64))


def _append_rows_args(X_new, factors, n_new, other, k, use_float):
    """The new rows of Session.append (include/poismf_hip.h section 2d), checked without a device as the library itself checks them:
    X_new a SciPy sparse matrix with one row per new row and `other` columns (or None: n_new empty rows), coerced to CSR with
    duplicates summed and indices sorted, every value finite and > 0; factors [n x k] and finite, or None.  Returns (n, data real_t,
    indptr, indices, factors real_t) with uint64 index arrays; the three matrix entries are None without X_new."""
    import scipy.sparse as sp
    dt = _real_t(use_float)
    data = indptr = indices = None
    if X_new is not None:
        if not sp.issparse(X_new):
            raise ValueError("append: the new rows must be a SciPy sparse matrix with one row per new row")
        if X_new.shape[1] != other:
            raise ValueError(f"append: the new rows have {X_new.shape[1]} columns, the other dimension is {other}")
        csr = sp.csr_matrix(X_new)
        csr.sum_duplicates(); csr.sort_indices()
        n = csr.shape[0]
        if n_new is not None and int(n_new) != n:
            raise ValueError(f"append: n_new = {n_new} but the new rows are {n}")
        data = np.ascontiguousarray(csr.data, dtype=dt)
        if not (np.isfinite(data).all() and (data > 0).all()):
            raise ValueError("append: every value must be finite and > 0")
        indptr, indices = np.ascontiguousarray(csr.indptr, dtype=np.uint64), np.ascontiguousarray(csr.indices, dtype=np.uint64)
    elif n_new is not None:
        if isinstance(n_new, bool) or not isinstance(n_new, (int, np.integer)) or n_new < 0:
            raise ValueError(f"append: n_new must be a non-negative integer, not {n_new!r}")
        n = int(n_new)
    elif factors is not None:
        n = np.shape(factors)[0] if np.ndim(factors) == 2 else -1
    else:
        raise ValueError("append: give the new rows, or n_new empty rows")
    if factors is not None:
        if np.ndim(factors) != 2 or np.shape(factors) != (n, k):
            raise ValueError(f"append: factors must have shape ({max(n, 0)}, {k}), not {np.shape(factors)}")
        factors = np.ascontiguousarray(factors, dtype=dt)
        if not np.isfinite(factors).all():
            raise ValueError("append: factors must be finite")
    return n, data, indptr, indices, factors


def _new_stats(Bsum, Amean, k, use_float):
    """Bsum (with l1 already added) and Amean of the fold-in calls as C-contiguous real_t k-vectors"""
    dt = _real_t(use_float)
    Bsum, Amean = np.ascontiguousarray(Bsum, dtype=dt).reshape(-1), np.ascontiguousarray(Amean, dtype=dt).reshape(-1)
    if len(Bsum) != k or len(Amean) != k:
        raise ValueError(f"Bsum and Amean must have k = {k} entries")
    return Bsum, Amean


def _topn_deep_args(users, n, exclude, dimA, dimB):
    """The argument checks of the deep batched top-N (include/poismf_hip.h section 1l) that need no device, as the library itself
    makes them: n up to TOPN_DEEP_MAX_N_TOP, and it may exceed what a user has left (short rows are padded).  Returns (users,
    excl_indptr or None, excl_indices or None) as uint64 arrays."""
    users, n = _users_and_n(users, n, api.TOPN_DEEP_MAX_N_TOP, "deep batched")
    _item_count(dimB)
    _users_in_range(users, dimA)
    return (users,) + _exclude_list(exclude, len(users), dimB)


def _topn_quota_args(users, n, group_of, quota, exclude, dimA, dimB):
    """The argument checks of the batched top-N with per-group quotas (include/poismf_hip.h section 1n) that need no device, as the
    library itself makes them: n up to TOPN_BATCH_MAX_N_TOP, and it may exceed what a user has left (short rows are padded).
    group_of: an integer array with one group id per item.  quota: one int for every group, or an array with one entry per group
    (its length is then the number of groups and must cover every id).  Returns (users, group_of, quota, excl_indptr or None,
    excl_indices or None) as uint64 arrays."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    _item_count(dimB, api.TOPN_QUOTA_MAX_ITEMS, "quota call")
    _users_in_range(users, dimA)
    if group_of is None:
        raise ValueError("group_of is required: one group id per item")
    group_of = _index_array(group_of, "group_of")
    if len(group_of) != dimB:
        raise ValueError(f"group_of has {len(group_of)} entries for {dimB} items")
    need = int(group_of.max()) + 1
    if quota is None:
        raise ValueError("quota is required: one int for every group, or one entry per group")
    if np.ndim(quota) == 0:
        if isinstance(quota, (bool, np.bool_)) or not isinstance(quota, (int, np.integer)):
            raise ValueError("quota must be integers")
        if int(quota) < 0:
            raise ValueError("quota: negative entry")
        quota = np.full(need, min(int(quota), 2**63), np.uint64)
    else:
        quota = _index_array(quota, "quota")
        if len(quota) < need:
            raise ValueError(f"quota has {len(quota)} entries, group_of names group {need - 1}")
    if len(quota) > 2**31 - 1:
        raise ValueError("there are more groups than the quota call supports (2^31 - 1)")
    return (users, group_of, quota) + _exclude_list(exclude, len(users), dimB)


def _topn_adjusted_args(users, n, adjust, exclude, dimA, dimB, dtype=np.float64):
    """The argument checks of the batched top-N with per-(user, item) score factors (include/poismf_hip.h section 1r) that need no
    device, as the library itself makes them: n up to TOPN_BATCH_MAX_N_TOP, and it may exceed what a user has left (short rows are
    padded).  adjust: None (no cell listed), a SciPy sparse matrix with one row per user of the batch whose stored values are the
    factors -- stored zeros are KEPT: a factor of 0 is a factor -- or an (indptr, indices, factors) triple; a row's indices strictly
    ascending (a sparse matrix is sorted first) and at most TOPN_ADJUSTED_MAX_ROW of them.  The factors are converted to `dtype`,
    the model's real_t, and must be finite and non-negative AFTER that conversion (a double above float32's range is refused for a
    float32 model).  Returns (users, adj_indptr, adj_indices, adj_factor, excl_indptr or None, excl_indices or None): uint64 arrays
    and the factors in `dtype`."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    m = len(users)
    _item_count(dimB, api.TOPN_ADJUSTED_MAX_ITEMS, "adjusted call")
    _users_in_range(users, dimA)
    if adjust is None:
        pair, f = (np.zeros(m + 1, np.uint64), np.zeros(0, np.uint64)), np.zeros(0, dtype)
    elif isinstance(adjust, (tuple, list)) and not hasattr(adjust, "tocsr"):
        if len(adjust) != 3:
            raise ValueError("adjust must be a SciPy sparse matrix or an (indptr, indices, factors) triple")
        pair, f = (adjust[0], adjust[1]), np.asarray(adjust[2])
    else:
        import scipy.sparse as sp
        if not sp.issparse(adjust):
            raise ValueError("adjust must be a SciPy sparse matrix or an (indptr, indices, factors) triple")
        csr = sp.csr_matrix(adjust)
        if csr.shape[0] != m:
            raise ValueError(f"adjust has {csr.shape[0]} rows for {m} users")
        if csr.shape[1] > dimB:
            raise ValueError("adjust has more columns than there are items")
        if not csr.has_sorted_indices:
            csr = csr.copy()
            csr.sort_indices()          # (stored zeros stay; a cell stored twice fails the ascending check below)
        pair, f = (csr.indptr, csr.indices), csr.data
    if f.ndim != 1 or (f.size and f.dtype.kind not in "fiu"):
        raise ValueError("adjust: the factors must be a 1-d array of real numbers")
    a_indptr, a_indices = _csr_list(pair, m, dimB, "adjust", row_max=api.TOPN_ADJUSTED_MAX_ROW)   # (from 0; the factors follow below)
    lo = int(np.asarray(pair[0]).reshape(-1)[0])
    hi = lo + int(a_indptr[-1])
    if len(f) < hi:
        raise ValueError("adjust: there are fewer factors than item indices")
    f = _finite_nonneg(f[lo:hi], dtype, "adjust: NaN factor", "adjust: a factor is",
                       "adjust: negative factor (a factor of 0 keeps a cell at score 0; exclude= bars one)")
    return (users, a_indptr, a_indices, f) + _exclude_list(exclude, m, dimB)


def _topn_weighted_args(users, n, item_weight, exclude, dimA, dimB, dtype=np.float64):
    """The argument checks of the batched top-N with per-item score weights (include/poismf_hip.h section 1o) that need no device, as
    the library itself makes them: n up to TOPN_BATCH_MAX_N_TOP, and it may exceed what a user has left (short rows are padded).
    item_weight: a 1-d array with one weight per item, or one number for all; converted to `dtype`, the model's real_t, and finite
    and non-negative AFTER that conversion (a double above float32's range is refused for a float32 model).  Returns (users,
    item_weight, excl_indptr or None, excl_indices or None): uint64 arrays around the weights in `dtype`."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    _item_count(dimB, api.TOPN_WEIGHTED_MAX_ITEMS, "weighted call")
    _users_in_range(users, dimA)
    if item_weight is None:
        raise ValueError("item_weight is required: one weight per item, or one number for all")
    w = np.asarray(item_weight)
    if w.dtype.kind not in "fiu":
        raise ValueError("item_weight must be real numbers")
    if w.ndim == 0:
        w = np.full(dimB, w)
    elif w.ndim != 1:
        raise ValueError("item_weight must be a 1-d array with one weight per item, or one number")
    if len(w) != dimB:
        raise ValueError(f"item_weight has {len(w)} entries for {dimB} items")
    w = _finite_nonneg(w, dtype, "item_weight: NaN entry", "item_weight: an entry is",
                       "item_weight: negative entry (a weight of 0 keeps an item at score 0; exclude= bars one)")
    return (users, w) + _exclude_list(exclude, len(users), dimB)


def _inv_norms(n2, dimB, dtype):
    """similar_items: inv[j] = real_t(1) / sqrt(n2[j]) in real_t, 0 where n2[j] == 0; n2[j] is the fused chain of B[j] with itself"""
    n2 = np.ascontiguousarray(n2, dtype=dtype).reshape(-1)
    if len(n2) != dimB:
        raise ValueError(f"item_norm has {len(n2)} entries for {dimB} items")
    if not np.isfinite(n2).all() or (n2 < 0).any():
        raise ValueError("item_norm must be finite and non-negative: the squared norms of the rows of B")
    inv = np.zeros(dimB, dtype)
    np.divide(dtype(1), np.sqrt(n2), out=inv, where=n2 != 0)
    return inv


def _topn_diverse_args(users, n, pool, lam, inv_norm, exclude, dimA, dimB, dtype=np.float64):
    """The argument checks of the diversified batched top-N (include/poismf_hip.h section 1p) that need no device, as the library
    itself makes them: n in 1 .. TOPN_BATCH_MAX_N_TOP, pool in n .. TOPN_DEEP_MAX_N_TOP (either may exceed what a user has left: short
    rows are padded), lam in [0, 1], and inv_norm -- _inv_norms' array, one entry per item -- finite and non-negative in `dtype`, the
    model's real_t.  Returns (users, inv_norm, excl_indptr or None, excl_indices or None): uint64 arrays around the norms in `dtype`."""
    users = _index_array(users, "users")
    n, pool = int(n), int(pool)
    _top_n(n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    if pool < n:
        raise ValueError(f"pool = {pool} is below n = {n}: the picks are made among the pool")
    if pool > api.TOPN_DEEP_MAX_N_TOP:
        raise ValueError(f"pool = {pool} is above the deep batched limit of {api.TOPN_DEEP_MAX_N_TOP}")
    if isinstance(lam, (bool, np.bool_)) or not isinstance(lam, (int, float, np.integer, np.floating)):
        raise ValueError("lam must be a real number in [0, 1]")
    if not 0.0 <= float(lam) <= 1.0:   # (NaN fails both)
        raise ValueError(f"lam = {lam} is outside [0, 1]")
    _item_count(dimB, api.TOPN_DIVERSE_MAX_ITEMS, "diversified call")
    _users_in_range(users, dimA)
    if inv_norm is None:
        raise ValueError("the items' inverse norms are required: one per item")
    inv = np.asarray(inv_norm)
    if inv.dtype.kind not in "fiu" or inv.ndim != 1:
        raise ValueError("the items' inverse norms must be a 1-d array of real numbers")
    if len(inv) != dimB:
        raise ValueError(f"there are {len(inv)} inverse norms for {dimB} items")
    inv = _finite_nonneg(inv, dtype, "inverse norm: NaN entry", "inverse norm: an entry is", "inverse norm: negative entry")
    return (users, inv) + _exclude_list(exclude, len(users), dimB)


def _similar_args(items, n, exclude_self, dimB):
    """similar_items: the query items as uint64 and the exclusion lists that leave each query itself out (or None); n, the items and
    the number of items are checked here, before any norm is computed"""
    items, n = _users_and_n(items, n, api.TOPN_BATCH_MAX_N_TOP, "batched", what="items")
    _item_count(dimB, api.TOPN_WEIGHTED_MAX_ITEMS, "weighted call", empty_ok=True)
    if len(items) and int(items.max()) >= dimB:
        raise ValueError("an item index is out of range")
    if not exclude_self:
        return items, None
    return items, (np.arange(len(items) + 1, dtype=np.uint64), items.copy())


def _similar_scores(sc, inv, items):
    """similar_items: wscore * inv[query] in real_t, a second rounded multiplication; padded entries stay -inf"""
    if sc.size:
        q = inv[items.astype(np.int64)][:, None]
        np.multiply(sc, q, out=sc, where=np.isfinite(sc))
    return sc


def _topn_include_args(users, n, include, exclude, dimA, dimB):
    """The argument checks of the batched top-N over include lists (include/poismf_hip.h section 1h) that need no device, as the
    library itself makes them: n may exceed what a user has left (short rows are padded).  Returns (users, incl_indptr,
    incl_indices, excl_indptr or None, excl_indices or None) as uint64 arrays."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    m = len(users)
    _users_in_range(users, dimA)
    ip, ii = _csr_list(include, m, dimB, "include", api.TOPN_INCLUDE_MAX_ROW, keep_zeros=True)
    return (users, ip, ii) + _exclude_list(exclude, m, dimB)


def _shared_table_args(include, include_of, m, dimB):
    """A table of lists shared between users and every user's row of it (include/poismf_hip.h sections 1i and 1k), checked without a
    device as the library itself checks them: `include` is the table (any number of rows G >= 1), include_of an integer array with
    one entry per user, or one int for all.  Returns (list_indptr, list_indices, list_of) as uint64 arrays."""
    if include is None:
        raise ValueError("include_of needs include, the table of lists it refers to")
    if isinstance(include, (tuple, list)) and len(include) == 2 and not hasattr(include, "tocsr"):
        G = max(len(np.asarray(include[0]).reshape(-1)) - 1, 0)
    elif hasattr(include, "shape") and len(include.shape) == 2:
        G = int(include.shape[0])
    else:
        raise ValueError("include must be a SciPy sparse matrix or an (indptr, indices) pair")
    if G < 1:
        raise ValueError("include: the table of lists has no rows")
    lp, li = _csr_list(include, G, dimB, "include", keep_zeros=True)
    if len(li) > api.TOPN_SHARED_MAX_CELLS:
        raise ValueError(f"include: the table of lists holds more than {api.TOPN_SHARED_MAX_CELLS} indices")
    if isinstance(include_of, (bool, np.bool_)):
        raise ValueError("include_of must be integers")
    if isinstance(include_of, (int, np.integer)):
        if include_of < 0:
            raise ValueError("include_of: negative index")
        lof = np.full(m, int(include_of), np.uint64)
    else:
        if np.ndim(include_of) != 1:
            raise ValueError("include_of must be a 1-d array with one entry per user, or one int")
        lof = _index_array(include_of, "include_of")
    if len(lof) != m:
        raise ValueError(f"include_of has {len(lof)} entries for {m} users")
    if m and int(lof.max()) >= G:
        raise ValueError(f"an entry of include_of is not a row of include ({G} lists)")
    return lp, li, lof


def _topn_shared_args(users, n, include, include_of, exclude, dimA, dimB):
    """The argument checks of the batched top-N over lists shared between users (include/poismf_hip.h section 1i) that need no
    device, as the library itself makes them: `include` is the table of lists (any number of rows G >= 1), include_of names every
    user's row of it (an integer array with one entry per user, or one int for all).  Returns (users, list_indptr, list_indices,
    list_of, excl_indptr or None, excl_indices or None) as uint64 arrays."""
    users, n = _users_and_n(users, n, api.TOPN_BATCH_MAX_N_TOP, "batched")
    m = len(users)
    _users_in_range(users, dimA)
    return (users,) + _shared_table_args(include, include_of, m, dimB) + _exclude_list(exclude, m, dimB)


def _rank_include_list(include, m, dimB):
    """The include lists of the batched ranks (include/poismf_hip.h section 1j), checked as the library checks them: (incl_indptr,
    incl_indices) as uint64 arrays"""
    return _csr_list(include, m, dimB, "include", api.TOPN_INCLUDE_MAX_ROW, keep_zeros=True)


def _rank_batch_args(users, test, exclude, dimA, dimB, k):
    """The argument checks of the batched ranks (include/poismf_hip.h sections 1g and 1j) that need no device, as the library itself
    makes them; returns (users, test_indptr, test_indices, excl_indptr or None, excl_indices or None) as uint64 arrays."""
    users = _index_array(users, "users")
    m = len(users)
    _users_in_range(users, dimA)
    if not 1 <= int(k) <= 512:
        raise ValueError("the number of factors is outside what the batched entry points support")
    if test is None:
        raise ValueError("the held-out list is missing")
    tp, ti = _csr_list(test, m, dimB, "test", api.RANK_BATCH_MAX_ROW)
    if exclude is None:
        return users, tp, ti, None, None
    ep, ei = _csr_list(exclude, m, dimB, "exclude", (api.RANK_BATCH_BUDGET_MB << 20) // 8)
    return users, tp, ti, ep, ei


def _eval_ranking_args(X_test, exclude, users, k, dimA, dimB):
    """eval_ranking's inputs, given for the whole matrix, cut down to the batch: (users, the (indptr, indices) of their held-out rows,
    their exclude rows or None, k)"""
    import scipy.sparse as sp
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    if not sp.issparse(X_test):
        raise ValueError("X_test must be a SciPy sparse matrix")
    if X_test.shape != (dimA, dimB):
        raise ValueError(f"X_test has shape {X_test.shape}, the model {(dimA, dimB)}")
    csr = sp.csr_matrix(X_test)
    csr.sum_duplicates()
    csr.eliminate_zeros()
    if users is None:
        users = np.flatnonzero(np.diff(csr.indptr)).astype(np.uint64)
    else:
        users = _index_array(users, "users")
        _users_in_range(users, dimA)
    rows = users.astype(np.int64)
    if exclude is not None and sp.issparse(exclude):
        if exclude.shape != (dimA, dimB):
            raise ValueError(f"exclude has shape {exclude.shape}, the model {(dimA, dimB)}")
        exclude = sp.csr_matrix(exclude)[rows]
    test = csr[rows]
    test.sort_indices()
    return users, (np.asarray(test.indptr, np.uint64), np.asarray(test.indices, np.uint64)), exclude, k


def _include_rows(include, users, dimA, dimB):
    """eval_ranking's include=, given either for the whole matrix (a sparse matrix of the model's shape, whose rows for `users` are
    taken) or for the batch (an (indptr, indices) pair with one row per user): the batch's (indptr, indices), checked"""
    import scipy.sparse as sp
    if sp.issparse(include):
        if include.shape != (dimA, dimB):
            raise ValueError(f"include has shape {include.shape}, the model {(dimA, dimB)}")
        include = sp.csr_matrix(include)[users.astype(np.int64)]
    return _rank_include_list(include, len(users), dimB)


def _include_of_rows(include_of, users, dimA):
    """eval_ranking's include_of=, given for the whole model (one int, or an integer array with one entry per user of the model,
    indexed by user id): what rank_batch takes -- the int itself, or the entries of `users`"""
    if isinstance(include_of, (bool, np.bool_)):
        raise ValueError("include_of must be integers")
    if isinstance(include_of, (int, np.integer)):
        return include_of
    if np.ndim(include_of) != 1:
        raise ValueError("include_of must be a 1-d array with one entry per user of the model, or one int")
    lof = _index_array(include_of, "include_of")
    if len(lof) != dimA:
        raise ValueError(f"include_of has {len(lof)} entries, the model {dimA} users")
    return lof[users.astype(np.int64)]


def _unite_rows(a, b):
    """Row by row, the union of two CSR-shaped lists with strictly ascending rows and the same number of rows: (indptr, indices) as
    uint64 arrays, rows strictly ascending.  No device is involved."""
    ap, ai = np.asarray(a[0], np.int64), np.asarray(a[1], np.int64)
    bp, bi = np.asarray(b[0], np.int64), np.asarray(b[1], np.int64)
    if len(ap) != len(bp):
        raise ValueError("the two lists have different numbers of rows")
    m = len(ap) - 1
    ai, bi = ai[ap[0]:ap[-1]], bi[bp[0]:bp[-1]]
    if len(ai) and int(ai.max()) >= 2 ** 32 or len(bi) and int(bi.max()) >= 2 ** 32:
        raise ValueError("an item index is out of range")
    rows = np.concatenate((np.repeat(np.arange(m, dtype=np.int64), np.diff(ap)), np.repeat(np.arange(m, dtype=np.int64), np.diff(bp))))
    key = np.unique((rows << 32) | np.concatenate((ai, bi)))      # one sort: (row, item) ascending, repeats merged
    rows, items = key >> 32, key & (2 ** 32 - 1)
    indptr = np.zeros(m + 1, np.uint64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return indptr, np.ascontiguousarray(items, dtype=np.uint64)


def _list_rows(items, dimB):
    """The lists of the list-wise evaluation (include/poismf_hip.h section 1q), checked as the library checks them: a 2-d integer
    array [m x n], 1 <= n <= TOPN_BATCH_MAX_N_TOP, whose rows hold distinct items below dimB followed only by TOPN_NONE -- what every
    topN_* call returns.  Returns it as a C-contiguous uint64 array."""
    a = np.asarray(items)
    if a.ndim != 2:
        raise ValueError("the lists must be a 2-d array with one row per user")
    if a.dtype.kind not in "iu":
        raise ValueError("the lists must hold integers")
    m, n = a.shape
    if n < 1:
        raise ValueError("the lists have no column")
    if n > api.TOPN_BATCH_MAX_N_TOP:
        raise ValueError(f"lists of {n} items are above the batched limit of {api.TOPN_BATCH_MAX_N_TOP}")
    if a.dtype.kind == "i" and a.size and int(a.min()) < 0:
        raise ValueError("the lists: negative index (an empty entry is TOPN_NONE)")
    a = np.ascontiguousarray(a, dtype=np.uint64)
    real = a != api.TOPN_NONE
    if np.any(real[:, 1:] & ~real[:, :-1]):
        raise ValueError("the lists: an item follows an empty entry of its row")
    if np.any(a[real] >= dimB):
        raise ValueError("an item index of the lists is out of range")
    if n > 1:
        srt = np.sort(a, axis=1)
        if np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != api.TOPN_NONE)):
            raise ValueError("the lists: a row names an item twice")
    return a


def _list_eval_scratch(m, n, cells, dimB, budget_bytes, real_size):
    """poismf_hip_list_eval_scratch_bytes, the same arithmetic on the host (include/poismf_hip.h section 1q): the one scratch
    allocation of a call in bytes, 0 when budget_bytes is below what the norms, the counts, one user and its cells need.  Returns
    (bytes, users per chunk, cells per chunk)."""
    up = lambda v: (v + 31) // 32 * 32
    m, n = max(int(m), 1), min(max(int(n), 1), api.TOPN_BATCH_MAX_N_TOP)
    dimB = min(max(int(dimB), 1), api.LIST_EVAL_MAX_ITEMS)
    full = api.LIST_EVAL_BUDGET_MB << 20
    budget = full if budget_bytes == 0 or budget_bytes > full else int(budget_bytes)
    fixed = up(dimB * real_size) + up(dimB * 4) + 256 + 4
    per_user = 4 * n + 16
    row_cells = min(int(cells), api.RANK_BATCH_MAX_ROW)
    if budget < fixed + per_user + row_cells * 8:
        return 0, 0, 0
    room = budget - fixed
    cell_cap = min(int(cells), max(row_cells, room // 2 // 8))
    chunk = min(m, (room - cell_cap * 8) // per_user, 262144)
    total = 0
    for part in (dimB * real_size, dimB * 4, chunk * n * 4, (chunk + 1) * 4, cell_cap * 4, cell_cap * 4, chunk * 8, chunk * 4):
        total = up(total + part)
    return total, chunk, cell_cap


def _list_eval_args(items, test, item_norm, budget_mb, dimB, k, dtype):
    """The argument checks of the list-wise evaluation (section 1q) that need no device, as the library itself makes them.  Returns
    (lists uint64 [m x n], test_indptr or None, test_indices or None, inverse norms in `dtype` or None, budget in bytes, 0 for the
    default)."""
    _item_count(dimB, api.LIST_EVAL_MAX_ITEMS, "list evaluation")
    if not 1 <= int(k) <= (512 if dtype == np.float32 else 256):
        raise ValueError("the number of factors is outside what the batched entry points support")
    lists = _list_rows(items, dimB)
    m, n = lists.shape
    tp = ti = None
    if test is not None:
        tp, ti = _csr_list(test, m, dimB, "test", api.RANK_BATCH_MAX_ROW)
    inv = None
    if item_norm is not None:
        if np.asarray(item_norm).dtype.kind not in "fiu":
            raise ValueError("item_norm must be real numbers")
        with np.errstate(over="ignore"):
            inv = _inv_norms(item_norm, dimB, dtype)
        # (1 / sqrt of a finite norm >= 0 is neither NaN nor negative: only the middle refusal can fire)
        inv = _finite_nonneg(inv, dtype, "item_norm: NaN inverse norm", "item_norm: an inverse norm is", "item_norm: negative inverse norm")
    budget = 0
    if budget_mb is not None:
        if isinstance(budget_mb, (bool, np.bool_)) or not isinstance(budget_mb, (int, float, np.integer, np.floating)):
            raise ValueError("budget_mb must be a positive number")
        if not float(budget_mb) > 0 or not np.isfinite(float(budget_mb)):
            raise ValueError("budget_mb must be a positive number")
        budget = max(int(float(budget_mb) * 2**20), 1)
    if _list_eval_scratch(m, n, len(ti) if ti is not None else 0, dimB, budget, np.dtype(dtype).itemsize)[0] == 0:
        raise ValueError(f"budget_mb = {budget_mb} is below what the norms, the counts and one user need")
    return lists, tp, ti, inv, budget


def _list_eval_outputs(lists, ti, inv, dimB):
    m = lists.shape[0]
    return (np.empty(len(ti), np.uint32) if ti is not None else None, np.empty(m, np.int64) if inv is not None else None,
            np.zeros(m, np.uint32), np.zeros(dimB, np.uint32))


def _eval_lists_args(items, users, X_test, k, exclude, item_pop, dimA, dimB):
    """eval_lists' inputs cut down to the batch: (lists uint64 [m x k], the (indptr, indices) of the held-out rows with every
    excluded cell removed, or None; item_pop as float64, or None)"""
    import scipy.sparse as sp
    lists = _list_rows(items, dimB)
    m, width = lists.shape
    if k is not None:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError("k must be an integer")
        if not 1 <= int(k) <= width:
            raise ValueError(f"k = {k} is outside 1 .. {width}, the lists' width")
        lists = np.ascontiguousarray(lists[:, :int(k)])
    if users is None:
        if (X_test is not None or exclude is not None) and m != dimA:
            raise ValueError(f"without users= the lists must have one row per user of the model: {m} rows for {dimA} users")
        users = np.arange(m, dtype=np.uint64)
    else:
        users = _index_array(users, "users")
        if len(users) != m:
            raise ValueError(f"there are {m} lists for {len(users)} users")
        _users_in_range(users, dimA)
    rows = users.astype(np.int64)
    if item_pop is not None:
        item_pop = np.asarray(item_pop)
        if item_pop.ndim != 1 or item_pop.dtype.kind not in "fiu" or len(item_pop) != dimB:
            raise ValueError(f"item_pop must be a 1-d array of real numbers with one entry per item ({dimB})")
        item_pop = item_pop.astype(np.float64)
        if not np.isfinite(item_pop).all() or (item_pop < 0).any():
            raise ValueError("item_pop must be finite and non-negative")
    test = None
    if X_test is not None:
        if not sp.issparse(X_test):
            raise ValueError("X_test must be a SciPy sparse matrix")
        if X_test.shape != (dimA, dimB):
            raise ValueError(f"X_test has shape {X_test.shape}, the model {(dimA, dimB)}")
        csr = sp.csr_matrix(X_test)
        csr.sum_duplicates()
        csr.eliminate_zeros()
        t = csr[rows]
        t.sort_indices()
        tp, ti = np.asarray(t.indptr, np.int64), np.asarray(t.indices, np.int64)
        if exclude is not None:
            if sp.issparse(exclude):
                if exclude.shape != (dimA, dimB):
                    raise ValueError(f"exclude has shape {exclude.shape}, the model {(dimA, dimB)}")
                exclude = sp.csr_matrix(exclude)[rows]
            ep, ei = _exclude_list(exclude, m, dimB)
            trow = np.repeat(np.arange(m, dtype=np.int64), np.diff(tp))
            erow = np.repeat(np.arange(m, dtype=np.int64), np.diff(ep.astype(np.int64)))
            keep = ~np.isin((trow << 32) | ti, (erow << 32) | ei.astype(np.int64))
            tp = np.concatenate(([0], np.cumsum(np.bincount(trow[keep], minlength=m)))).astype(np.int64)
            ti = ti[keep]
        test = (tp.astype(np.uint64), ti.astype(np.uint64))
    elif exclude is not None:
        raise ValueError("exclude removes held-out cells: it needs X_test")
    return lists, test, item_pop


# ---- the one call path --------------------------------------------------------------------------------------------------------------

def _topn_call(target, name, users, n, middle, exclude_seen, excl, output_score, output_value=None):
    """What every batched top-N call does once its arguments are checked, on either target: the shard check of exclude_seen, the
    output arrays (three with output_value, the diversified call's), the early return without users -- before anything of a library
    is touched -- and the call itself: the target's leading arguments, users, m, n, the variant's middle arguments (`middle()`,
    asked for only now; `tuple` where a variant has none), the session's exclude_seen flag, the exclusion lists, the outputs."""
    m, dt = len(users), _real_t(target.use_float)
    if exclude_seen:
        _outside_shard(users, target.shardA)
    out = _topn_outputs(m, n, dt, output_score) if output_value is None else _diverse_outputs(m, n, dt, output_score, output_value)
    if m == 0:
        return out
    fn, lead, flag = target._entry(name, exclude_seen)
    _batch_rc(fn(*lead, _ptr(users), m, n, *middle(), *flag, _opt_ptr(excl[0]), _opt_ptr(excl[1]), _ptr(out[0]),
                 *map(_opt_ptr, out[1:])), "top-N")
    return out


def topn_batch(target, users, n, exclude_seen, exclude, output_score, include, include_of):
    """sections 1f, 1h and 1i: plain, over a list per user (include), over a table of lists shared between users (include_of)"""
    if include_of is not None:
        users, lp, li, lof, *excl = _topn_shared_args(users, n, include, include_of, exclude, target.dimA, target.dimB)
        name, middle = "topn_shared", lambda: (_ptr(lp), _opt_ptr(li), len(lp) - 1, _ptr(lof))
    elif include is not None:
        users, ip, ii, *excl = _topn_include_args(users, n, include, exclude, target.dimA, target.dimB)
        name, middle = "topn_include", lambda: (_ptr(ip), _opt_ptr(ii))
    else:
        users, *excl = _topn_batch_args(users, n, exclude, target.dimA, target.dimB)
        name, middle = "topn_batch", tuple
    return _topn_call(target, name, users, int(n), middle, exclude_seen, excl, output_score)


def topn_deep(target, users, n, exclude_seen, exclude, output_score):
    """section 1l"""
    users, *excl = _topn_deep_args(users, n, exclude, target.dimA, target.dimB)
    return _topn_call(target, "topn_deep", users, int(n), tuple, exclude_seen, excl, output_score)


def topn_quota(target, users, n, group_of, quota, exclude_seen, exclude, output_score):
    """section 1n"""
    users, group_of, quota, *excl = _topn_quota_args(users, n, group_of, quota, exclude, target.dimA, target.dimB)
    return _topn_call(target, "topn_quota", users, int(n), lambda: (_ptr(group_of), len(quota), _ptr(quota)), exclude_seen, excl,
                      output_score)


def topn_weighted(target, users, n, item_weight, exclude_seen, exclude, output_score, query_items=None):
    """section 1o.  query_items: None on host factors, whose entry point has no such argument; on a session the flag that makes
    `users` rows of the resident B, which goes in front of exclude_seen."""
    if query_items and exclude_seen:
        raise ValueError("exclude_seen has no meaning with query_items: the session holds no seen rows for items")
    users, w, *excl = _topn_weighted_args(users, n, item_weight, exclude, target.dimB if query_items else target.dimA, target.dimB,
                                          _real_t(target.use_float))
    flag = () if query_items is None else (int(bool(query_items)),)
    return _topn_call(target, "topn_weighted", users, int(n), lambda: (_ptr(w),) + flag, exclude_seen, excl, output_score)


def similar_items(target, items, n, output_score, exclude_self, item_norm, query_items=None):
    """similar_items of both classes: the weighted call with rows of B as the queries -- host factors hold B in both places, a
    session is told by query_items -- under the inverse norms as weights, then _similar_scores"""
    items, excl = _similar_args(items, n, exclude_self, target.dimB)
    inv = _inv_norms(target.item_norms() if item_norm is None else item_norm, target.dimB, _real_t(target.use_float))
    ix, sc = topn_weighted(target, items, n, inv, False, excl, output_score, query_items)
    return ix, _similar_scores(sc, inv, items)


def topn_adjusted(target, users, n, adjust, exclude_seen, exclude, output_score):
    """section 1r"""
    users, a_indptr, a_indices, f, *excl = _topn_adjusted_args(users, n, adjust, exclude, target.dimA, target.dimB,
                                                               _real_t(target.use_float))
    return _topn_call(target, "topn_adjusted", users, int(n), lambda: (_ptr(a_indptr), _opt_ptr(a_indices), _opt_ptr(f)), exclude_seen,
                      excl, output_score)


def topn_diverse(target, users, n, pool, lam, exclude_seen, exclude, output_score, output_value, item_norm):
    """section 1p.  Everything else is judged before the norms are computed: zeros stand in for them until there are users."""
    dt = _real_t(target.use_float)
    inv = np.zeros(target.dimB, dt) if item_norm is None else _inv_norms(item_norm, target.dimB, dt)
    users, inv, *excl = _topn_diverse_args(users, n, pool, lam, inv, exclude, target.dimA, target.dimB, dt)

    def middle():
        norms = inv if item_norm is not None else _inv_norms(target.item_norms(), target.dimB, dt)
        return int(pool), float(lam), _ptr(norms)

    return _topn_call(target, "topn_diverse", users, int(n), middle, exclude_seen, excl, output_score, bool(output_value))


def rank_batch(target, users, test, exclude_seen, exclude, include, include_of, unite_test):
    """sections 1g, 1j and 1k: among all items, among a list per user (include), among a table of lists shared between users
    (include_of) -- the ranks' counterpart of topn_batch and _topn_call, in the same order"""
    users, tp, ti, ep, ei = _rank_batch_args(users, test, exclude, target.dimA, target.dimB, target.k)
    m = len(users)
    name, middle = "rank_batch", ()
    if include_of is not None:
        lp, li, lof = _shared_table_args(include, include_of, m, target.dimB)
        name, middle = "rank_shared", (_ptr(lp), _opt_ptr(li), len(lp) - 1, _ptr(lof), int(bool(unite_test)))
    elif unite_test:
        raise ValueError("unite_test needs include_of: a list per user has its held-out row united in by the caller")
    elif include is not None:
        ip, ii = _rank_include_list(include, m, target.dimB)
        name, middle = "rank_include", (_ptr(ip), _opt_ptr(ii))
    if exclude_seen:
        _outside_shard(users, target.shardA)
    ranks, n_adm = np.empty(len(ti), np.uint32), np.empty(m, np.uint32)
    if m == 0:
        return ranks, n_adm
    fn, lead, flag = target._entry(name, exclude_seen)
    _batch_rc(fn(*lead, _ptr(users), m, _ptr(tp), _opt_ptr(ti), *middle, *flag, _opt_ptr(ep), _opt_ptr(ei), _ptr(ranks), _ptr(n_adm)),
              "ranks")
    return ranks, n_adm


from . import api   # noqa: E402  (at the end: api imports this module while it is being loaded itself, and is only used in calls)
