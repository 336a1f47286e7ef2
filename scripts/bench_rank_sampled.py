#!/usr/bin/env python3
"""Time the sampled ranks in one pass (include/poismf_hip.h section 1u) against the two calls they replace.

    python scripts/bench_rank_sampled.py [--out profiles/rank_sampled/bench.json] [--repeats 5]
    python scripts/bench_rank_sampled.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_sample_negatives.py: dimA 10^6, dimB 10^5, k 50, fp32, a uniform CSR (synth) of 10^7 cells whose rows
are the seen items (exclude_seen), and ten held-out cells per user drawn uniformly (repeats and seen cells dropped, so a few rows
hold nine).  Method as there: a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of
timed work per figure, the two routes alternated inside each repeat; median (min .. max).

    fused_<shape>      Session.rank_sampled(users, test, m, exclude_seen=True[, item_weight=counts], seed=...)
    two_step_<shape>   what eval_ranking(negatives=) did before: Session.sample_negatives(users, m, exclude_seen=True, exclude=test, ...),
                       the held-out rows united into the sample on the host, Session.rank_batch(users, test, exclude_seen=True,
                       include=<that>)
    shapes: 4096x100, 4096x1000, allx100 (10^6 users), popular_4096x1000 (item weights = the items' counts in the CSR)

Asserted at every shape: the two routes return identical ranks and n_adm.  No ratio is asserted: the ratio is what this measures.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from poismf_amd import api, serving, synth
from scripts.bench_topn_include import stat, timed


def held_out(rng, dimA, dimB, seen_keys, per_user=10):
    """(indptr, indices) uint64: per user up to per_user distinct unseen items, ascending"""
    cand = np.sort(rng.integers(0, dimB, (dimA, per_user)), axis=1)
    keys = np.arange(dimA, dtype=np.int64)[:, None] * dimB + cand
    at = np.minimum(np.searchsorted(seen_keys, keys), len(seen_keys) - 1)
    keep = seen_keys[at] != keys
    keep[:, 1:] &= cand[:, 1:] != cand[:, :-1]
    return np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.uint64), cand[keep].astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_sampled", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k = args.dimA, args.dimB, args.k
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    rng = np.random.default_rng(1)
    sess.set_factors(rng.random((dimA, k), dtype=np.float32), rng.random((dimB, k), dtype=np.float32))
    _, indices, indptr = sess.matrix(1)
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    seen_keys = np.repeat(np.arange(dimA, dtype=np.int64), np.diff(indptr)) * dimB + indices
    counts = np.bincount(indices, minlength=dimB).astype(np.uint32)
    tp, ti = held_out(rng, dimA, dimB, seen_keys)
    everyone, few = np.arange(dimA, dtype=np.uint64), min(4096, dimA)
    shapes = [("4096x100", few, 100, None), ("4096x1000", few, 1000, None), ("allx100", dimA, 100, None), ("popular_4096x1000", few, 1000, counts)]

    def fused(n, m, w):
        return sess.rank_sampled(everyone[:n], (tp[:n + 1], ti[:int(tp[n])]), m, exclude_seen=True, item_weight=w, seed=17)

    def two_step(n, m, w):
        users, test = everyone[:n], (tp[:n + 1], ti[:int(tp[n])])
        sample = sess.sample_negatives(users, m, exclude_seen=True, exclude=test, item_weight=w, seed=17)
        return sess.rank_batch(users, test, exclude_seen=True, include=serving._unite_rows(serving._rank_include_list(sample, n, dimB), test))

    if args.trace_pass:
        for _ in range(3):
            for _, n, m, w in shapes:
                if n == few:
                    fused(n, m, w)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": [s[0] for s in shapes if s[1] == few]}))
        return

    paths, same = [], {}
    for name, n, m, w in shapes:
        paths.append(("fused_" + name, lambda n=n, m=m, w=w: fused(n, m, w), n, n * m))
        paths.append(("two_step_" + name, lambda n=n, m=m, w=w: two_step(n, m, w), n, n * m))
        a, b = paths[-2][1](), paths[-1][1]()                                     # (the first call of every shape doubles as its warm-up)
        same[name] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), held_out_cells=int(tp[-1]), exclude_seen=True, precision="fp32"),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; routes alternated; median of repeats",
           "device": torch.cuda.get_device_name(0), "identical_ranks_and_n_adm": same}
    for name, _, n, cells in paths:
        out[name] = stat(ms[name], n, cells)
        if name.startswith("two_step_"):
            out["two_step_over_fused_" + name[9:]] = out[name]["ms"] / out["fused_" + name[9:]]["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert all(same.values()), same


if __name__ == "__main__":
    main()
