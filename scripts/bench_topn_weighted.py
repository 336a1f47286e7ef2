#!/usr/bin/env python3
"""Time the batched top-N with per-item score weights (include/poismf_hip.h section 1o) against the plain call and against the route
it replaces, and the similar-items call built on it.

    python scripts/bench_topn_weighted.py [--out profiles/topn_weighted/bench_topn_weighted.json] [--nnz 10000000] [--repeats 5]

scripts/bench_topn.py's workload and method: dimA 10^6, dimB 10^5, k = 50, fp32, random positive factors, a uniform CSR (synth),
n_top = 10, seen items excluded; a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of
timed work per figure, five repeats with the paths alternated inside each repeat; median, min and max reported.  The weights are
log-uniform in [1/4, 4).

    weighted_4096, weighted_all   Session.topn_weighted(exclude_seen=True) for the first 4096 users / all 10^6; with them the share of
                                  rows that differ from Session.topn_batch's
    ones_4096, ones_all           every weight 1, next to plain_4096 / plain_all (Session.topn_batch on the same users in the same
                                  process): the ratio is the price of the epilogue and of the upload.  Recorded, not asserted
    deep_route_4096               today's only route: Session.topn_deep(users, 1000, exclude_seen=True), the 1000 scores per user times
                                  the weights and re-ranked on the host.  It cannot see an item the weight lifts from beyond place 1000:
                                  the share of rows on which it is WRONG (differs from weighted_4096's items) is reported
    similar_4096                  Session.similar_items for the first 4096 items, item_norm= computed once beforehand (item_norms_ms:
                                  that one computation, which brings the factors to the host)

Asserted: weighted_4096 is faster than deep_route_4096.  Nothing else.
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


def host_reweight(ix, sc, weight, n_top):
    """the weights applied on the host to ranked lists [m x depth] (TOPN_NONE pads a short one): every row's n_top best entries under
    (score x weight descending, item ascending).  Returns (items, weighted scores)."""
    real = ix != api.TOPN_NONE
    safe = np.where(real, ix, 0).astype(np.int64)
    ws = np.where(real, np.multiply(sc, weight[safe]), -np.inf).astype(sc.dtype)
    by_item = np.argsort(np.where(real, ix, api.TOPN_NONE), axis=1, kind="stable")
    ws_i = np.take_along_axis(ws, by_item, 1)
    by_score = np.argsort(-ws_i, axis=1, kind="stable")[:, :n_top]          # (stable: ties stay in item order)
    pick = np.take_along_axis(by_item, by_score, 1)
    return np.take_along_axis(ix, pick, 1), np.take_along_axis(ws, pick, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_weighted", "bench_topn_weighted.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-users", type=int, default=4096)
    args = ap.parse_args()
    dimA, dimB, k, n_top, m = args.dimA, args.dimB, args.k, 10, args.head_users
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    users = np.arange(m, dtype=np.uint64)
    items = np.arange(min(m, dimB), dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)
    weight = np.exp(rng.uniform(np.log(0.25), np.log(4.0), dimB)).astype(np.float32)
    ones = np.ones(dimB, np.float32)
    t0 = time.perf_counter()
    n2 = sess.item_norms()
    item_norms_ms = (time.perf_counter() - t0) * 1e3
    res = {}

    def weighted_call(who, w):
        return sess.topn_weighted(who, n_top, item_weight=w, exclude_seen=True, output_score=True)

    def plain_call(who):
        return sess.topn_batch(who, n_top, exclude_seen=True, output_score=True)

    def weighted_4096():
        res["weighted_4096"] = weighted_call(users, weight)

    def weighted_all():
        res["weighted_all"] = weighted_call(everyone, weight)

    def ones_4096():
        res["ones_4096"] = weighted_call(users, ones)

    def ones_all():
        res["ones_all"] = weighted_call(everyone, ones)

    def plain_4096():
        res["plain_4096"] = plain_call(users)

    def plain_all():
        res["plain_all"] = plain_call(everyone)

    def deep_route_4096():
        ix, sc = sess.topn_deep(users, 1000, exclude_seen=True, output_score=True)
        res["deep_route_4096"] = host_reweight(ix, sc, weight, n_top)

    def similar_4096():
        res["similar_4096"] = sess.similar_items(items, n_top, output_score=True, item_norm=n2)

    paths = [("weighted_4096", weighted_4096, m), ("ones_4096", ones_4096, m), ("plain_4096", plain_4096, m), ("deep_route_4096", deep_route_4096, m),
             ("similar_4096", similar_4096, len(items)), ("weighted_all", weighted_all, dimA), ("ones_all", ones_all, dimA), ("plain_all", plain_all, dimA)]
    for _, fn, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, head_users=m,
                            item_weight="log-uniform in [1/4, 4)"),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0), "item_norms_ms": item_norms_ms}
    for name, _, nu in paths:
        out[name] = figure(ms[name], nu)
    for size in ("4096", "all"):
        out[f"weighted_{size}"]["share_of_rows_differing_from_topn_batch"] = float(
            (res[f"weighted_{size}"][0] != res[f"plain_{size}"][0]).any(axis=1).mean())
        out[f"ones_{size}"]["ms_over_topn_batch_ms"] = out[f"ones_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
        out[f"weighted_{size}"]["ms_over_topn_batch_ms"] = out[f"weighted_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
        out[f"ones_{size}"]["rows_equal_topn_batch"] = bool(np.array_equal(res[f"ones_{size}"][0], res[f"plain_{size}"][0]) and
                                                            res[f"ones_{size}"][1].tobytes() == res[f"plain_{size}"][1].tobytes())
    d_ix, d_sc = res["deep_route_4096"]
    w_ix, w_sc = res["weighted_4096"]
    wrong = (d_ix != w_ix).any(axis=1)
    out["deep_route_4096"]["share_of_rows_wrong"] = float(wrong.mean())
    out["deep_route_4096"]["rows_wrong"] = int(wrong.sum())
    out["deep_route_4096"]["right_rows_equal_weighted_4096_bits"] = bool(d_sc[~wrong].tobytes() == w_sc[~wrong].tobytes())
    out["speedup_weighted_4096_over_deep_route"] = out["deep_route_4096"]["ms"] / out["weighted_4096"]["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert out["speedup_weighted_4096_over_deep_route"] > 1.0, out["speedup_weighted_4096_over_deep_route"]


if __name__ == "__main__":
    main()
