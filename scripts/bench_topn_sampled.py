#!/usr/bin/env python3
"""Time the sampled top-N (include/poismf_hip.h section 1w) against the route it replaces and against the weighted call with weights of
one, and report what the sampled page does to exposure.

    python scripts/bench_topn_sampled.py [--out profiles/topn_sampled/bench.json] [--nnz 10000000] [--repeats 5]
    python scripts/bench_topn_sampled.py --trace-pass   # what to put under `rocprofv3 --kernel-trace --stats -- ...`: three calls per path, no timing

scripts/bench_topn_weighted.py's workload and method: dimA 10^6, dimB 10^5, k = 50, fp32, random positive factors, a uniform CSR (synth),
n_top = 10, seen items excluded, T = 1; a device-synchronised host clock around whole calls, every shape warmed up first, five repeats
with the paths alternated inside each repeat; median, min and max reported.  A figure is ONE call where a call takes 0.5 s or more.

    sampled_4096, sampled_all   Session.topn_sampled(exclude_seen=True) for the first 4096 users / all 10^6
    ones_4096, ones_all         Session.topn_weighted with every weight 1 on the same users: the tile kernel without the drawing
                                epilogue, so the difference is the epilogue's cost
    deep_route_4096             the route before: Session.topn_deep(users, 1000, exclude_seen=True), the same keys made with numpy for the
                                1000 listed items and re-ranked on the host.  It cannot draw an item beyond place 1000: the share of
                                rows on which it differs from sampled_4096's items is reported
    exposure                    eval_lists' coverage and Gini of sampled_all's pages beside the plain pages' (Session.topn_batch)

No target is asserted: the figures are reported.  Not timed: fp64, other k, other n, other T.
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
from scripts.bench_topn_weighted import figure, timed

MASK = np.uint64(2 ** 32 - 1)


def host_factors(seed, users, items, T):
    """r(u, j) of section 1w in float64 for items [m x depth] of the users: Philox in uint64 arithmetic, log1p and power"""
    u = np.asarray(users, np.uint64)[:, None] + 0 * items
    c = [items >> np.uint64(2), np.ones_like(items), u & MASK, u >> np.uint64(32)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    word = np.take_along_axis(np.stack(c), (items & np.uint64(3)).astype(np.int64)[None], axis=0)[0]
    return np.power(-np.log1p(-(word.astype(np.float64) + 0.5) / 2.0 ** 32), -T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_sampled", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-users", type=int, default=4096)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, n_top, m, T, seed = args.dimA, args.dimB, args.k, 10, args.head_users, 1.0, 7
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    users = np.arange(m, dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)
    ones = np.ones(dimB, np.float32)
    res = {}

    def sampled_4096():
        res["sampled_4096"] = sess.topn_sampled(users, n_top, T, seed, exclude_seen=True, output_score=True)

    def sampled_all():
        res["sampled_all"] = sess.topn_sampled(everyone, n_top, T, seed, exclude_seen=True, output_score=True)

    def ones_4096():
        res["ones_4096"] = sess.topn_weighted(users, n_top, item_weight=ones, exclude_seen=True, output_score=True)

    def ones_all():
        res["ones_all"] = sess.topn_weighted(everyone, n_top, item_weight=ones, exclude_seen=True, output_score=True)

    def deep_route_4096():
        ix, sc = sess.topn_deep(users, 1000, exclude_seen=True, output_score=True)
        real = ix != api.TOPN_NONE
        r = np.where(real, host_factors(seed, users, np.where(real, ix, 0), T), 0.0)
        keys = np.where(real, sc.astype(np.float64) * r, -np.inf)
        res["deep_route_4096"] = np.take_along_axis(ix, np.argsort(-keys, axis=1, kind="stable")[:, :n_top], 1)

    if args.trace_pass:
        for _ in range(3):
            for fn in (sampled_4096, ones_4096, sampled_all, ones_all):
                fn()
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_per_path": 3}))
        return

    paths = [("sampled_4096", sampled_4096, m, 0.5), ("ones_4096", ones_4096, m, 0.5), ("deep_route_4096", deep_route_4096, m, 0.0),
             ("sampled_all", sampled_all, dimA, 0.0), ("ones_all", ones_all, dimA, 0.0)]
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, min_s in paths:
            ms[name].append(timed(fn, min_s))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, head_users=m, temperature=T, seed=seed),
           "method": "host clock around whole calls between device synchronisations; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0), "not_timed": "fp64, other k, other n, other T"}
    for name, _, nu, _ in paths:
        out[name] = figure(ms[name], nu)
    for size in ("4096", "all"):
        out[f"sampled_{size}"]["ms_over_ones_ms"] = out[f"sampled_{size}"]["ms"] / out[f"ones_{size}"]["ms"]
    wrong = (res["deep_route_4096"] != res["sampled_4096"][0]).any(axis=1)
    out["deep_route_4096"]["share_of_rows_differing_from_exact"] = float(wrong.mean())
    out["speedup_sampled_4096_over_deep_route"] = out["deep_route_4096"]["ms"] / out["sampled_4096"]["ms"]
    plain = sess.topn_batch(everyone, n_top, exclude_seen=True)[0]
    n2 = sess.item_norms()
    for name, pages in (("plain", plain), ("sampled", res["sampled_all"][0])):
        ev = sess.eval_lists(pages, item_norm=n2)
        out[f"exposure_{name}"] = dict(coverage=float(ev["coverage"]), gini=float(ev["gini"]))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
