"""Ranking metrics from exact ranks (include/poismf_hip.h section 1g).  numpy only: nothing here touches a device.

The ranks come from PoisMF.eval_ranking / Session.rank_batch: for every held-out cell of a user, the 0-based position of its item
in the user's complete ranked list over the N admissible items ("score descending, item index ascending").  These are the
project's own definitions.  For a user whose valid ranks in ascending order are r_0 < r_1 < ... < r_{p-1} (p >= 1), N = n_adm and
cut-off K = k:

    hit         1 if r_0 < K else 0
    precision   #{r_i < K} / K
    recall      #{r_i < K} / p
    ap          (1 / min(K, p)) * sum over r_i < K of (i + 1) / (r_i + 1)
    ndcg        sum over r_i < K of 1 / log2(r_i + 2), divided by sum_{i < min(K, p)} 1 / log2(i + 2)
    rr          1 / (r_0 + 1) if r_0 < K else 0
    auc         1 - sum_i (r_i - i) / (p (N - p)): the share of (held-out, other) pairs of admissible items in the right order;
                NaN when N == p

A cell marked RANK_EXCLUDED (its item is in the user's exclusion set) takes no part.  A user without a valid cell gets NaN
everywhere and is left out of the means.
"""
import warnings

import numpy as np

RANK_EXCLUDED = 0xFFFFFFFF   # the header's rank of an excluded cell (tests/test_rank_batch_cpu.py compares the two)
METRICS = ("hit", "precision", "recall", "ap", "ndcg", "rr", "auc")


def metrics_from_ranks(test_indptr, ranks, n_adm, k):
    """Per-user float64 arrays of the seven metrics (a dict keyed by METRICS) for m = len(test_indptr) - 1 users: row i of the
    CSR-shaped held-out list owns ranks[test_indptr[i]:test_indptr[i + 1]] (any order) and n_adm[i] admissible items."""
    indptr = np.asarray(test_indptr).astype(np.int64)
    ranks = np.asarray(ranks).astype(np.int64)
    N = np.asarray(n_adm).astype(np.int64)
    K = int(k)
    if K < 1:
        raise ValueError("k must be at least 1")
    m = len(indptr) - 1
    if m < 0 or len(N) != m or (m and (indptr[0] != 0 or np.any(indptr[1:] < indptr[:-1]))) or (len(ranks) != (indptr[-1] if m else 0)):
        raise ValueError("test_indptr, ranks and n_adm do not fit together")
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    valid = ranks != RANK_EXCLUDED
    r, rw = ranks[valid], rows[valid]
    order = np.lexsort((r, rw))            # by user, ranks ascending within a user
    r, rw = r[order], rw[order]
    p = np.bincount(rw, minlength=m).astype(np.int64)
    start = np.cumsum(p) - p
    i = np.arange(len(r), dtype=np.int64) - start[rw]      # the rank's place among the user's own
    top = r < K
    has = p > 0
    pf = np.where(has, p, 1).astype(np.float64)

    def per_user(weights):
        return np.bincount(rw[top], weights=weights[top], minlength=m) if len(r) else np.zeros(m)

    hits = per_user(np.ones(len(r)))
    best = np.full(m, np.iinfo(np.int64).max)
    best[has] = r[start[has]]
    cut = np.minimum(K, np.where(has, p, 1))               # min(K, p)
    ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(int(cut.max()) if m else 0, dtype=np.float64) + 2.0))))
    out = {
        "hit": (best < K).astype(np.float64),
        "precision": hits / K,
        "recall": hits / pf,
        "ap": per_user((i + 1.0) / (r + 1.0)) / cut,
        "ndcg": per_user(1.0 / np.log2(r + 2.0)) / ideal[cut],
        "rr": np.where(best < K, 1.0 / (np.where(has, best, 0) + 1.0), 0.0),
    }
    others = p * (N - p)                                    # (held-out, other) pairs
    wrong = np.bincount(rw, weights=(r - i).astype(np.float64), minlength=m) if len(r) else np.zeros(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["auc"] = np.where(others > 0, 1.0 - wrong / others, np.nan)
    for name in METRICS:
        out[name] = np.where(has, out[name], np.nan)
    return out


def nan_mean(x):
    """The mean of the entries that are not NaN; NaN, quietly, when there is none."""
    x = np.asarray(x, np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # (a mean over no user is NaN, quietly)
        return float(np.nanmean(x)) if len(x) else float("nan")


def mean_metrics(per_user, names=METRICS):
    """The means over the users that counted (NaN entries left out), plus n_users: how many had a valid held-out cell."""
    out = {name: nan_mean(per_user[name]) for name in names}
    out["n_users"] = int(np.count_nonzero(~np.isnan(per_user["hit"])))
    return out


# ---- list-wise evaluation (include/poismf_hip.h section 1q): the metrics of GIVEN lists, from PoisMF.eval_lists / api.list_eval ----
LIST_ABSENT = 0xFFFFFFFE     # the header's position of a held-out item its list lacks (tests/test_list_eval_cpu.py compares the two)
LIST_COS_SHIFT = 40          # cos_sum counts cosines in units of 2^-40
LIST_METRICS = ("hit", "precision", "recall", "ap", "ndcg", "rr")


def metrics_from_positions(test_indptr, pos, k):
    """Per-user float64 arrays of the six list metrics (a dict keyed by LIST_METRICS) for m = len(test_indptr) - 1 lists of k items:
    row i of the CSR-shaped held-out list owns pos[test_indptr[i]:test_indptr[i + 1]], each the 0-based position of a held-out item
    in the user's list or LIST_ABSENT.  The definitions are those at the top of this module with the position as the rank r, K = k
    and p = ALL the user's held-out cells: an absent cell has a rank beyond any cut-off, so it adds to no sum and still counts in p
    (recall = listed held-out items / held-out items; ap and ndcg divide by min(K, p)).  A user whose cells are all absent gets 0
    everywhere, a user without a cell NaN, left out of the means.  There is no auc: a list says nothing about the order of the
    items it lacks."""
    pos = np.asarray(pos).astype(np.int64)
    if np.any((pos >= int(k)) & (pos != LIST_ABSENT)) or np.any(pos < 0):
        raise ValueError("a position lies outside the list")
    # (LIST_ABSENT is itself a rank beyond every cut-off and is not RANK_EXCLUDED; n_adm plays a part in auc only)
    each = metrics_from_ranks(test_indptr, pos, np.zeros(max(len(np.asarray(test_indptr)) - 1, 0), np.int64), k)
    return {name: each[name] for name in LIST_METRICS}


def ild(cos_sum, length):
    """Intra-list diversity per list: ild[u] = 1 - (cos_sum[u] / 2^LIST_COS_SHIFT) / (c (c - 1) / 2) with c = length[u], one minus the
    mean cosine over the list's pairs of items (the cosine of similar_items; section 1q sums it in fixed point).  NaN for c < 2."""
    c = np.asarray(length).astype(np.float64)
    pairs = c * (c - 1.0) / 2.0
    s = np.asarray(cos_sum).astype(np.float64) / 2.0 ** LIST_COS_SHIFT
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(pairs > 0, 1.0 - s / np.where(pairs > 0, pairs, 1.0), np.nan)


def coverage(exposure):
    """count_nonzero(exposure) / dimB: the share of the catalogue that some list shows"""
    x = np.asarray(exposure)
    return float(np.count_nonzero(x)) / len(x) if len(x) else float("nan")


def gini(exposure):
    """The Gini coefficient of the exposure counts: with x ascending, N = dimB and i 1-based, sum_i (2 i - N - 1) x_i / (N sum_i x_i);
    0 when every item is shown equally often, (N - 1) / N when one item takes everything.  NaN when nothing was shown."""
    x = np.sort(np.asarray(exposure).astype(np.float64))
    N = len(x)
    total = x.sum() if N else 0.0
    if not total > 0:
        return float("nan")
    return float(((2.0 * np.arange(1, N + 1) - N - 1.0) * x).sum() / (N * total))


def novelty(items, item_pop, none=2 ** 64 - 1):
    """Per list, the mean over its real entries (those that are not `none`, TOPN_NONE) of -log2(max(item_pop[j], 1) / sum(item_pop)):
    the self-information of the items under the popularity counts item_pop.  NaN for a list without an entry."""
    items = np.asarray(items)
    pop = np.asarray(item_pop).astype(np.float64)
    real = items != np.asarray(none, dtype=items.dtype) if items.dtype.kind == "u" else items >= 0
    info = -np.log2(np.maximum(pop, 1.0) / pop.sum()) if pop.sum() > 0 else np.full(len(pop), np.nan)
    each = np.where(real, info[np.where(real, items, 0).astype(np.int64)], 0.0)
    c = real.sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, each.sum(axis=1) / np.where(c > 0, c, 1.0), np.nan)
