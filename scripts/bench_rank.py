#!/usr/bin/env python3
"""Time the batched exact ranks (include/poismf_hip.h section 1g) against the batched top-N on the same users.

    python scripts/bench_rank.py [--out profiles/rank/bench_rank.json] [--nnz 10000000] [--repeats 5]
    python scripts/bench_rank.py --trace-pass        # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_topn.py: dimA 10^6, dimB 10^5, k = 50, fp32, random positive factors, a uniform CSR (synth), seen
items excluded; ten held-out cells per user.  Four cases: (a) the first 4096 users and (b) all users, each with two placements of
the held-out cells, which bracket what a fitted model gives:

    uniform   drawn uniformly from the items: AUC near 0.5, most scores fall between a user's thresholds -- the epilogue's worst case
    top       drawn from the user's own best 128 as Session.topn_batch lists them: nearly every score dies in registers -- the best case

The yardstick is Session.topn_batch(users, 10, exclude_seen=True) on the same users in the same process; the dense pass of the
ranks does the same multiplications.  Figures: a device-synchronised host clock around whole Session.rank_batch calls (argument
checks, uploads, the five kernels and downloads included), every shape warmed up first, at least 0.5 s of timed work, five
repeats, the paths alternated inside each repeat; median, min and max, and the ratio of each case's median to its yardstick's.
The kernels' own times come from the trace pass.
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

from poismf_amd import api, metrics, synth

CELLS = 10


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


def uniform_cells(rng, m, dimB):
    """CELLS distinct uniformly drawn items per user, ascending: (indptr, indices)"""
    ix = np.sort(rng.integers(0, dimB, (m, CELLS)), axis=1)
    for r in np.flatnonzero((ix[:, 1:] == ix[:, :-1]).any(axis=1)):   # (the few rows that drew an item twice)
        ix[r] = np.sort(rng.choice(dimB, CELLS, replace=False))
    return np.arange(m + 1, dtype=np.uint64) * CELLS, ix.reshape(-1).astype(np.uint64)


def top_cells(rng, sess, users):
    """CELLS of every user's best 128 admissible items, ascending"""
    out = np.empty((len(users), CELLS), np.uint64)
    for lo in range(0, len(users), 1 << 16):
        top, _ = sess.topn_batch(users[lo:lo + (1 << 16)], 128, exclude_seen=True)
        pick = np.argpartition(rng.random(top.shape), CELLS, axis=1)[:, :CELLS]
        out[lo:lo + len(top)] = np.sort(np.take_along_axis(top, pick, axis=1), axis=1)
    indptr = np.arange(len(users) + 1, dtype=np.uint64) * CELLS
    return indptr, out.reshape(-1)


def summary(ms_list):
    return dict(ms=float(np.median(ms_list)), ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), repeats=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank", "bench_rank.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--few-users", type=int, default=4096)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, m = args.dimA, args.dimB, args.k, args.few_users
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    del trip
    few = np.arange(m, dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)
    cells = {("few", "uniform"): uniform_cells(rng, m, dimB), ("all", "uniform"): uniform_cells(rng, dimA, dimB),
             ("few", "top"): top_cells(rng, sess, few), ("all", "top"): top_cells(rng, sess, everyone)}
    batch = {"few": few, "all": everyone}
    last = {}

    def rank_call(which, place):
        def fn():
            last[(which, place)] = sess.rank_batch(batch[which], cells[(which, place)], exclude_seen=True)
        return fn

    def topn_call(which):
        return lambda: sess.topn_batch(batch[which], 10, exclude_seen=True)

    paths = [(f"rank_{which}_{place}", rank_call(which, place)) for which in ("few", "all") for place in ("uniform", "top")]
    paths += [("topn_few", topn_call("few")), ("topn_all", topn_call("all"))]

    if args.trace_pass:
        for _ in range(2):
            for _, fn in paths:
                fn()
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 2}))
        return

    for _, fn in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _ in paths}
    for _ in range(args.repeats):
        for name, fn in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), exclude_seen=True, few_users=m, cells_per_user=CELLS),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _ in paths:
        out[name] = summary(ms[name])
    for which in ("few", "all"):
        for place in ("uniform", "top"):
            name = f"rank_{which}_{place}"
            out[name]["ratio_to_topn"] = out[name]["ms"] / out[f"topn_{which}"]["ms"]
            ranks, n_adm = last[(which, place)]
            t0 = time.perf_counter()
            mean = metrics.mean_metrics(metrics.metrics_from_ranks(cells[(which, place)][0], ranks, n_adm, 10))
            out[name]["metrics_host_ms"] = (time.perf_counter() - t0) * 1e3
            out[name]["auc"], out[name]["ndcg"], out[name]["largest_rank"] = mean["auc"], mean["ndcg"], int(ranks[ranks != api.RANK_EXCLUDED].max())
    # the placements are what they claim to be
    assert 0.49 < out["rank_all_uniform"]["auc"] < 0.51, out["rank_all_uniform"]["auc"]
    assert out["rank_all_top"]["largest_rank"] < 128 and out["rank_few_top"]["largest_rank"] < 128
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
