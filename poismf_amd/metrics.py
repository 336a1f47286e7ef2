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


def mean_metrics(per_user):
    """The means over the users that counted (NaN entries left out), plus n_users: how many had a valid held-out cell."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # (a mean over no user is NaN, quietly)
        for name in METRICS:
            out[name] = float(np.nanmean(per_user[name])) if len(per_user[name]) else float("nan")
    out["n_users"] = int(np.count_nonzero(~np.isnan(per_user["hit"])))
    return out
