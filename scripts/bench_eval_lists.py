#!/usr/bin/env python3
"""Time the list-wise evaluation (include/poismf_hip.h section 1q) against the only route there was before it, and put the plain and
the diversified page side by side.

    python scripts/bench_eval_lists.py [--out profiles/list_eval/bench_eval_lists.json] [--nnz 10000000] [--repeats 5] [--sizes 4096,1000000]

scripts/bench_topn_diverse.py's workload: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), seen items excluded, items in
families of ten near-duplicates (item j with j % 10 != 0 is item j - j % 10 with every entry moved by about two percent).  The two
pages of every user: Session.topn_batch(n = 10) and Session.topn_diverse(n = 10, pool = 100, lam = 0.7).  Held-out: ten cells per
user -- five drawn from the user's own plain top 20, five anywhere (fewer where two coincide) -- so that the hit metrics have
something to find; the factors are random, so the figures say what the re-ranking does to THESE pages, not to a fitted model.

Per size (the first 4096 users, all 10^6) and page, a device-synchronised host clock around whole calls, one warm-up, then the median
of --repeats single calls, the routes alternated inside each repeat:

    eval_lists   Session.eval_lists(items, users, X_test, item_norm=...): the held-out rows cut out of X_test on the host, one
                 poismf_hip_session_list_eval, the metrics in numpy
    list_eval    Session.list_eval on the rows already cut: the device call alone, lists and cells going up, four arrays coming back
    numpy        the same four arrays without the call, from a host copy of B (get_factors(), once, not timed): B[items], a batched
                 matmul, the two multiplications and the quantisation, bincount, searchsorted on (row, item) keys

The script asserts that positions, lengths and exposure of the two routes are identical; numpy's sums over k are not the fused
chain, so the cosine sums may differ by roundings: the largest difference in ild is reported, not asserted.  No ratio is asserted.
--trace makes five list_eval calls each on the diversified page, the plain page and a page of evenly spread items at the largest size
and writes no record: the run to put behind `rocprofv3 --kernel-trace --stats --`, in a run of its own.  The third page has no hot
item, so its kernel time beside the others' is what the contended exposure atomics cost.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
import torch

from poismf_amd import api, metrics, synth


def once(fn):
    """ms of one call of fn, between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def figure(ms_list, users):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3), repeats=len(ms_list))


def numpy_route(B, inv, items, tp, ti, step=65536):
    """section 1q's four outputs from host arrays: (pos, cos_sum, length, exposure).  The chains are numpy's sums over k."""
    m, n = items.shape
    real = items != api.TOPN_NONE
    safe = np.where(real, items, 0).astype(np.int64)
    length = real.sum(axis=1).astype(np.uint32)
    expo = np.bincount(safe[real], minlength=B.shape[0]).astype(np.uint32)
    cos = np.empty(m, np.int64)
    lower = np.tril(np.ones((n, n), bool), -1)
    for u0 in range(0, m, step):
        s, r = safe[u0:u0 + step], real[u0:u0 + step]
        rows = B[s]                                                        # [m x n x k]
        inv_r = np.where(r, inv[s], B.dtype.type(0))
        G = np.matmul(rows, rows.transpose(0, 2, 1))                       # [m x n x n], [q, p]
        cs = np.multiply(np.multiply(G, inv_r[:, :, None]), inv_r[:, None, :])
        t = cs.astype(np.float64)
        Q = np.rint(np.clip(np.where(np.isnan(t), 0, t), -2, 2) * 2.0 ** api.LIST_COS_SHIFT).astype(np.int64)
        cos[u0:u0 + step] = np.where(lower & r[:, :, None] & r[:, None, :], Q, 0).sum(axis=(1, 2))
    # positions: the (row, item) key of every cell looked up among the sorted keys of the lists' real entries
    row_of = np.repeat(np.arange(m, dtype=np.int64), n).reshape(m, n)
    keys = ((row_of << 32) | safe)[real]
    place = np.tile(np.arange(n, dtype=np.uint32), m).reshape(m, n)[real]
    order = np.argsort(keys, kind="stable")
    keys, place = keys[order], place[order]
    cell = (np.repeat(np.arange(m, dtype=np.int64), np.diff(tp.astype(np.int64))) << 32) | ti.astype(np.int64)
    at = np.minimum(np.searchsorted(keys, cell), max(len(keys) - 1, 0))
    pos = np.where(keys[at] == cell, place[at], np.uint32(api.LIST_ABSENT)).astype(np.uint32) if len(keys) else np.full(len(cell), api.LIST_ABSENT, np.uint32)
    return pos, cos, length, expo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_eval", "bench_eval_lists.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="4096,1000000")
    ap.add_argument("--trace", action="store_true", help="five list_eval calls on the diversified page and no record: the run a kernel trace is taken of")
    args = ap.parse_args()
    dimA, dimB, k = args.dimA, args.dimB, args.k
    sizes = [min(int(s), dimA) for s in args.sizes.split(",")]
    n_top, pool, lam = 10, 100, 0.7
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    head = np.arange(dimB) - np.arange(dimB) % 10
    B = np.where((np.arange(dimB) % 10 != 0)[:, None], B[head] * (1.0 + 0.02 * rng.standard_normal((dimB, k))), B).astype(np.float32)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    B_host = sess.get_factors()[1]                     # the baseline's copy of B: fetched once, not timed
    n2 = sess.item_norms()
    inv = api._inv_norms(n2, dimB, np.float32)
    m_max = max(sizes)
    everyone = np.arange(m_max, dtype=np.uint64)

    # the two pages and the held-out cells of the largest size; a smaller size takes their first rows
    step = 1 << 17
    pages = {"plain": np.empty((m_max, n_top), np.uint64), "diverse": np.empty((m_max, n_top), np.uint64)}
    top20 = np.empty((m_max, 20), np.uint64)
    for u0 in range(0, m_max, step):
        u = everyone[u0:u0 + step]
        top20[u0:u0 + step] = sess.topn_batch(u, 20, exclude_seen=True)[0]
        pages["diverse"][u0:u0 + step] = sess.topn_diverse(u, n_top, pool, lam, exclude_seen=True, item_norm=n2)[0]
    pages["plain"][:] = top20[:, :n_top]
    own = np.take_along_axis(top20, np.argsort(rng.random((m_max, 20)), axis=1)[:, :5].astype(np.int64), axis=1).astype(np.int64)
    cells = np.unique((np.repeat(np.arange(m_max, dtype=np.int64), 10) << 32) |
                      np.concatenate((own, rng.integers(0, dimB, (m_max, 5))), axis=1).reshape(-1))
    X_test = sp.csr_matrix((np.ones(len(cells), np.float32), ((cells >> 32), (cells & (2 ** 32 - 1)))), shape=(dimA, dimB))
    del top20, own, cells

    if args.trace:
        # five calls each, in this order, on the diversified page, the plain page and a page without a hot item -- row u lists items
        # (s_u + 9973 i) mod dimB, i = 0 .. 9, s_u uniform -- whose kernel does the same work with its exposure counts spread evenly:
        # the difference of the kernel times is what the contended atomics cost
        spread = ((rng.integers(0, dimB, (m_max, 1)) + 9973 * np.arange(n_top)) % dimB).astype(np.uint64)
        test = X_test[:m_max]
        for items in (pages["diverse"], pages["plain"], spread):
            for _ in range(5):
                expo = sess.list_eval(items, test, item_norm=n2)[3]
            print(f"hottest item: in {int(expo.max())} lists; items shown: {int(np.count_nonzero(expo))}", file=sys.stderr, flush=True)
        sess.close()
        return

    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, pool=pool, lam=lam, nnz=int(sess.nnz(1)), exclude_seen=True,
                            held_out_cells=int(X_test[:m_max].nnz),
                            items="families of ten: item j with j % 10 != 0 is item j - j % 10 with every entry moved by about 2 %",
                            held_out="per user five of its own plain top 20 and five items anywhere"),
           "method": "host clock around whole calls between device synchronisations; one warm-up, then the median of single calls; routes alternated",
           "device": torch.cuda.get_device_name(0), "not_timed": "fp64, k other than 50, lists wider than 10, more than one GPU"}
    for m in sizes:
        users = everyone[:m]
        test = X_test[:m]
        tp, ti = np.asarray(test.indptr, np.uint64), np.asarray(test.indices, np.uint64)
        rec = {}
        for page, items_all in pages.items():
            items = np.ascontiguousarray(items_all[:m])
            res = {}
            routes = [("eval_lists", lambda: res.__setitem__("eval_lists", sess.eval_lists(items, users, X_test, item_norm=n2, per_user=True))),
                      ("list_eval", lambda: res.__setitem__("list_eval", sess.list_eval(items, (tp, ti), item_norm=n2))),
                      ("numpy", lambda: res.__setitem__("numpy", numpy_route(B_host, inv, items, tp, ti)))]
            for _, fn in routes:
                fn()
            ms = {name: [] for name, _ in routes}
            for _ in range(args.repeats):
                for name, fn in routes:
                    ms[name].append(once(fn))
            dev, host = res["list_eval"], res["numpy"]
            assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[2], host[2]) and np.array_equal(dev[3], host[3]), (m, page)
            full = res["eval_lists"]
            assert np.array_equal(full["positions"], dev[0]) and np.array_equal(full["cos_sum"], dev[1])
            r = {name: figure(ms[name], m) for name, _ in routes}
            r["numpy_ms_over_list_eval_ms"] = r["numpy"]["ms"] / r["list_eval"]["ms"]
            r["largest_ild_difference_numpy_vs_device"] = float(np.nanmax(np.abs(metrics.ild(dev[1], dev[2]) - metrics.ild(host[1], host[2]))))
            r["cos_sums_identical"] = bool(np.array_equal(dev[1], host[1]))
            r["hottest_item_in_lists"] = int(dev[3].max())
            r["metrics"] = {name: full[name] for name in ("hit", "precision", "recall", "ap", "ndcg", "rr", "ild", "coverage", "gini", "n_users", "n_lists")}
            rec[page] = r
            print(f"{m} users, {page}: eval_lists {r['eval_lists']['ms']:.1f} ms, list_eval {r['list_eval']['ms']:.1f} ms, numpy {r['numpy']['ms']:.1f} ms",
                  file=sys.stderr, flush=True)
        rec["share_of_rows_the_diversified_page_changes"] = float((pages["plain"][:m] != pages["diverse"][:m]).any(axis=1).mean())
        out[f"users_{m}"] = rec
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
