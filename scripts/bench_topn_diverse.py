#!/usr/bin/env python3
"""Time the diversified batched top-N (include/poismf_hip.h section 1p) against the route it replaces, and its MMR stage against the
pool stage alone.

    python scripts/bench_topn_diverse.py [--out profiles/topn_diverse/bench_topn_diverse.json] [--nnz 10000000] [--repeats 5]

scripts/bench_topn_weighted.py's workload and method: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), seen items excluded,
the first 4096 users; a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of timed work
per figure, five repeats with the paths alternated inside each repeat; median, min and max reported.  So that diversification has
something to do, the items come in families of ten: item j with j % 10 != 0 is item j - j % 10 with every entry moved by about two
percent -- ten editions of one record.  n = 10, pool = 100, lam = 0.7.

    diverse_4096      Session.topn_diverse(exclude_seen=True, item_norm=...), and the share of rows that differ from Session.topn_batch's
                      (plain_4096, timed beside it)
    host_route_4096   today's only route: Session.topn_deep(users, pool, exclude_seen=True), then greedy MMR over the pools in numpy on
                      the host, vectorised over the users, from a host copy of B.  Its chains are numpy's sums, not the fused chain, so
                      a row may differ by a rounding: the share of identical rows is reported, and the ratio of the two times
    lam1_4096         the same call at lam = 1 next to deep_4096, Session.topn_deep(users, pool) alone: the difference is what the
                      MMR stage costs (and decides whether an LDS-resident pool is worth building)
    deep_pool_1000    n = 100 of pool = 1000, one timed call after a warm-up, beside Session.topn_deep(users, 1000)

Nothing is asserted about a ratio.  --trace makes 21 calls of diverse_4096 and writes no record: the run to put behind
`rocprofv3 --kernel-trace --stats --`, in a run of its own, for the kernels' own times.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from poismf_amd import api, synth


def timed(fn, min_s=0.5):
    """ms per call of fn: calls repeated until min_s of work is inside the window"""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / n * 1e3


def figure(ms_list, users):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3), repeats=len(ms_list))


def host_mmr(ix, sc, B, inv, n_top, lam):
    """section 1p's greedy loop over pools [m x p] (TOPN_NONE pads a short one) on the host, vectorised over the users, in the pools'
    precision; the chains are numpy's sums over k.  Returns (items, relevances, values), [m x n_top]."""
    dt = sc.dtype.type
    m, p = ix.shape
    real = ix != api.TOPN_NONE
    safe = np.where(real, ix, 0).astype(np.int64)
    rows = B[safe]                                                     # [m x p x k]
    inv_p = np.where(real, inv[safe], dt(0))
    first = sc[:, :1]
    r = np.where(first > 0, np.divide(sc, np.where(first > 0, first, dt(1))), sc)
    lr = np.multiply(dt(lam), r)
    oml = dt(1.0 - lam)
    mx = np.zeros((m, p), sc.dtype)
    free = real.copy()
    out_ix = np.full((m, n_top), api.TOPN_NONE, np.uint64)
    out_sc = np.full((m, n_top), -np.inf, sc.dtype)
    out_v = np.full((m, n_top), -np.inf, sc.dtype)
    every = np.arange(m)
    for t in range(n_top):
        v = np.where(free, np.subtract(lr, np.multiply(oml, mx)), -np.inf)
        q = np.argmax(v, axis=1)                                       # (the first of equal values: the lowest position)
        live = free[every, q]
        out_ix[live, t], out_sc[live, t], out_v[live, t] = ix[every, q][live], sc[every, q][live], v[every, q][live]
        free[every, q] = False
        chain = np.einsum("mpk,mk->mp", rows, rows[every, q])
        cs = np.multiply(np.multiply(chain, inv_p), inv_p[every, q][:, None])
        mx = np.where(cs > mx, cs, mx)
    return out_ix, out_sc, out_v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_diverse", "bench_topn_diverse.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-users", type=int, default=4096)
    ap.add_argument("--trace", action="store_true", help="21 calls of diverse_4096 and no record: the run a kernel trace is taken of")
    args = ap.parse_args()
    dimA, dimB, k, m = args.dimA, args.dimB, args.k, args.head_users
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
    users = np.arange(m, dtype=np.uint64)
    t0 = time.perf_counter()
    n2 = sess.item_norms()
    item_norms_ms = (time.perf_counter() - t0) * 1e3
    inv = api._inv_norms(n2, dimB, np.float32)
    res = {}

    def diverse_4096():
        res["diverse_4096"] = sess.topn_diverse(users, n_top, pool, lam, exclude_seen=True, output_score=True, output_value=True, item_norm=n2)

    def plain_4096():
        res["plain_4096"] = sess.topn_batch(users, n_top, exclude_seen=True, output_score=True)

    def host_route_4096():
        ix, sc = sess.topn_deep(users, pool, exclude_seen=True, output_score=True)
        res["host_route_4096"] = host_mmr(ix, sc, B, inv, n_top, lam)

    def lam1_4096():
        res["lam1_4096"] = sess.topn_diverse(users, n_top, pool, 1.0, exclude_seen=True, output_score=True, item_norm=n2)

    def deep_4096():
        res["deep_4096"] = sess.topn_deep(users, pool, exclude_seen=True, output_score=True)

    if args.trace:   # for `rocprofv3 --kernel-trace --stats -- python scripts/bench_topn_diverse.py --trace`: the headline call and nothing else
        for _ in range(21):
            diverse_4096()
        sess.close()
        return
    paths = [("diverse_4096", diverse_4096), ("plain_4096", plain_4096), ("host_route_4096", host_route_4096), ("lam1_4096", lam1_4096),
             ("deep_4096", deep_4096)]
    for _, fn in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _ in paths}
    for _ in range(args.repeats):
        for name, fn in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, pool=pool, lam=lam, nnz=int(sess.nnz(1)), exclude_seen=True, head_users=m,
                            items="families of ten: item j with j % 10 != 0 is item j - j % 10 with every entry moved by about 2 %"),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0), "item_norms_ms": item_norms_ms}
    for name, _ in paths:
        out[name] = figure(ms[name], m)
    d, h = res["diverse_4096"], res["host_route_4096"]
    out["diverse_4096"]["share_of_rows_differing_from_topn_batch"] = float((d[0] != res["plain_4096"][0]).any(axis=1).mean())
    out["diverse_4096"]["ms_over_topn_batch_ms"] = out["diverse_4096"]["ms"] / out["plain_4096"]["ms"]
    rows_equal = (d[0] == h[0]).all(axis=1)
    out["host_route_4096"]["share_of_rows_with_the_same_items"] = float(rows_equal.mean())
    out["host_route_4096"]["all_rows_identical"] = bool(rows_equal.all() and d[1].tobytes() == h[1].tobytes() and d[2].tobytes() == h[2].tobytes())
    out["speedup_diverse_4096_over_host_route"] = out["host_route_4096"]["ms"] / out["diverse_4096"]["ms"]
    out["lam1_4096"]["rows_equal_topn_deep_head"] = bool(np.array_equal(res["lam1_4096"][0], res["deep_4096"][0][:, :n_top]) and
                                                        res["lam1_4096"][1].tobytes() == np.ascontiguousarray(res["deep_4096"][1][:, :n_top]).tobytes())
    out["lam1_4096"]["ms_over_topn_deep_ms"] = out["lam1_4096"]["ms"] / out["deep_4096"]["ms"]
    out["mmr_stage_ms"] = out["lam1_4096"]["ms"] - out["deep_4096"]["ms"]
    out["mmr_stage_costs_more_than_pool_stage"] = bool(out["mmr_stage_ms"] > out["deep_4096"]["ms"])

    # n = 100 of pool = 1000: one timed call each, after a warm-up
    big = {}
    for name, fn in (("diverse", lambda: sess.topn_diverse(users, 100, 1000, lam, exclude_seen=True, item_norm=n2)),
                     ("deep", lambda: sess.topn_deep(users, 1000, exclude_seen=True))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        big[name + "_ms"] = (time.perf_counter() - t0) * 1e3
    out["deep_pool_1000"] = dict(n_top=100, pool=1000, repeats=1, **big)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
