#!/usr/bin/env python3
"""Time the negative sampler (include/poismf_hip.h section 1t) against the host route it replaces.

    python scripts/bench_sample_negatives.py [--out profiles/sample_negatives/bench.json] [--repeats 5]
    python scripts/bench_sample_negatives.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_topn_include.py: dimA 10^6, dimB 10^5, fp32, a uniform CSR (synth) of 10^7 cells whose rows are the
seen items; every sample excludes them (exclude_seen).  The factors play no part and are never set.  Method as there: a
device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of timed work per figure, repeats
with the paths alternated inside each repeat; median (min .. max).

    device_<w>_4096x1000 / 4096x100 / allx100   Session.sample_negatives(users, m, exclude_seen=True[, item_weight=counts], seed=...)
    host_<w>_...                                the same lists from numpy in this process, as vectorised as it gets: candidates drawn in
                                                bulk (numpy.random), seen cells masked by searchsorted on (row, item) keys, repeats
                                                within a row found by a stable sort, the first m survivors in draw order kept, short
                                                rows redrawn; blocks of 65 536 users bound its memory
    <w> is "uniform" or "popular" (item weights = the items' counts in the CSR).

The two routes cannot give the same bits (different generators), so what is asserted of BOTH, at every shape, is the contract's
shape: every row ascending, distinct, disjoint from the user's seen items and of length m.  No speed-up is asserted.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from poismf_amd import api, synth
from scripts.bench_topn_include import stat, timed


def host_sample(rng, users, m, dimB, seen_keys, cdf):
    """(indptr, indices): m distinct unseen items per user, rows ascending.  seen_keys: user * dimB + item of every seen cell, sorted"""
    out = np.empty((len(users), m), np.int64)
    for b0 in range(0, len(users), 65536):
        todo = np.arange(b0, min(b0 + 65536, len(users)))
        while len(todo):
            n, over = len(todo), int(m * 1.25) + 16
            cand = rng.integers(0, dimB, (n, over)) if cdf is None else np.searchsorted(cdf, rng.random((n, over)), side="right")
            keys = users[todo].astype(np.int64)[:, None] * dimB + cand
            at = np.minimum(np.searchsorted(seen_keys, keys), len(seen_keys) - 1)
            bad = seen_keys[at] == keys
            order = np.argsort(cand, axis=1, kind="stable")                       # equal candidates side by side, the earlier draw first
            sc = np.take_along_axis(cand, order, 1)
            rep = np.zeros_like(bad)
            rep[:, 1:] = sc[:, 1:] == sc[:, :-1]
            np.put_along_axis(bad, order, np.take_along_axis(bad, order, 1) | rep, 1)
            keep = ~bad & (np.cumsum(~bad, axis=1) <= m)                          # the first m survivors in draw order
            full = keep.sum(axis=1) == m
            out[todo[full]] = np.sort(cand[full][keep[full]].reshape(-1, m), axis=1)
            todo = todo[~full]                                                    # a short row is drawn again
    return np.arange(len(users) + 1, dtype=np.int64) * m, out.ravel()


def check(sample, users, m, dimB, seen_keys):
    """the contract's shape: rows of m, strictly ascending (hence distinct), below dimB, disjoint from the seen items"""
    indptr, items = sample[0], sample[1].astype(np.int64)
    rows = items.reshape(len(users), m)
    keys = (users.astype(np.int64)[:, None] * dimB + rows).ravel()
    at = np.minimum(np.searchsorted(seen_keys, keys), len(seen_keys) - 1)
    return bool(np.all(np.diff(indptr) == m) and np.all(rows[:, 1:] > rows[:, :-1]) and rows.max() < dimB and not np.any(seen_keys[at] == keys))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_negatives", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB = args.dimA, args.dimB
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    sess = api.Session.from_coo(trip, 4, True)
    del trip
    _, indices, indptr = sess.matrix(1)
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    seen_keys = np.repeat(np.arange(dimA, dtype=np.int64), np.diff(indptr)) * dimB + indices
    assert np.all(seen_keys[1:] > seen_keys[:-1])
    counts = np.bincount(indices, minlength=dimB).astype(np.uint32)
    cdf = np.cumsum(counts) / counts.sum()
    rng = np.random.default_rng(1)
    everyone = np.arange(dimA, dtype=np.uint64)
    shapes = [("4096x1000", everyone[:min(4096, dimA)], 1000), ("4096x100", everyone[:min(4096, dimA)], 100), ("allx100", everyone, 100)]

    def device(u, m, w):
        return sess.sample_negatives(u, m, exclude_seen=True, item_weight=counts if w == "popular" else None, seed=17)

    if args.trace_pass:
        for _ in range(3):
            for _, u, m in shapes[:2]:
                device(u, m, "uniform")
                device(u, m, "popular")
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": ["4096x1000", "4096x100"], "weights": ["uniform", "popular"]}))
        return

    paths, ok = [], {}
    for w in ("uniform", "popular"):
        for name, u, m in shapes:
            paths.append((f"device_{w}_{name}", lambda u=u, m=m, w=w: device(u, m, w), len(u), m * len(u)))
            paths.append((f"host_{w}_{name}", lambda u=u, m=m, w=w: host_sample(rng, u, m, dimB, seen_keys, cdf if w == "popular" else None), len(u),
                          m * len(u)))
            # (the first call of every shape doubles as its warm-up)
            ok[f"{w}_{name}"] = {"device": check(paths[-2][1](), u, m, dimB, seen_keys), "host": check(paths[-1][1](), u, m, dimB, seen_keys)}
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, nnz=int(sess.nnz(1)), exclude_seen=True),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0), "rows_ascending_distinct_unseen_of_length_m": ok}
    for name, _, nu, cells in paths:
        out[name] = stat(ms[name], nu, cells)
        if name.startswith("host_"):
            out["speedup_" + name[5:]] = out[name]["ms"] / out["device_" + name[5:]]["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert all(v for d in ok.values() for v in d.values()), ok


if __name__ == "__main__":
    main()
