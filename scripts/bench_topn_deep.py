#!/usr/bin/env python3
"""Time the deep batched top-N (include/poismf_hip.h section 1l) against the per-user loop it replaces and against the shallow call.

    python scripts/bench_topn_deep.py [--out profiles/topn_deep/bench_topn_deep.json] [--nnz 10000000] [--repeats 5]
    python scripts/bench_topn_deep.py --trace-pass   # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_topn.py: random positive factors, dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), seen items
excluded.  Figures (each: a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of timed
work, five repeats, the paths alternated inside each repeat; median, min and max reported):

    per_user_loop_n1000   Session.topn(u, 1000, exclude_ix = row u) over the first 4096 users -- the code that was there before
    deep_4096_n1000       the same users in one Session.topn_deep(exclude_seen=True) call
    deep_4096_n256, deep_4096_n128, batch_4096_n128 (Session.topn_batch: the price of lists in HBM, and where to switch)
    deep_262144_n256      262 144 users in one call; output_bytes is what that call returns

Whole-call rates (uploads, merge, downloads and the widening of the items to 64 bits included), not a kernel's share of peak: that
comes from the trace pass.  The condition the feature has to meet -- deep_4096_n1000 at least ten times faster than
per_user_loop_n1000 in the same process, rows right under tests.helpers.check_topn -- is asserted.
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

from poismf_amd import api, synth
from tests import helpers as H


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


def figure(ms_list, users, n_top):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3), users=users, n_top=n_top,
                output_bytes=users * n_top * (8 + 4), repeats=len(ms_list))   # (uint64 items and fp32 scores, as the caller gets them)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_deep", "bench_topn_deep.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=4096)
    ap.add_argument("--many-users", type=int, default=262144)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, m, many = args.dimA, args.dimB, args.k, args.loop_users, min(args.many_users, args.dimA)
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    users = np.arange(m, dtype=np.uint64)
    crowd = np.arange(many, dtype=np.uint64)

    if args.trace_pass:
        for _ in range(2):
            sess.topn_deep(users, 1000, exclude_seen=True, output_score=True)
            sess.topn_deep(users, 256, exclude_seen=True, output_score=True)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 2}))
        return

    head = trip.row < m
    X = sp.csr_matrix((np.ones(int(head.sum()), np.float32), (trip.row[head], trip.col[head])), shape=(m, dimB))
    X.sum_duplicates(); X.sort_indices()
    rows = [X.indices[X.indptr[u]:X.indptr[u + 1]].astype(np.uint64) for u in range(m)]
    del trip

    keep = {}

    def per_user_loop_n1000():
        ix = np.empty((m, 1000), np.uint64)
        sc = np.empty((m, 1000), np.float32)
        for u in range(m):
            ix[u], sc[u] = sess.topn(u, 1000, exclude_ix=rows[u], output_score=True)
        keep["loop"] = (ix, sc)

    def deep(who, n, tag=None):
        def run():
            out = sess.topn_deep(who, n, exclude_seen=True, output_score=True)
            if tag:
                keep[tag] = out
        return run

    def batch_4096_n128():
        keep["batch128"] = sess.topn_batch(users, 128, exclude_seen=True, output_score=True)

    paths = [("per_user_loop_n1000", per_user_loop_n1000, m, 1000), ("deep_4096_n1000", deep(users, 1000, "deep1000"), m, 1000),
             ("deep_4096_n256", deep(users, 256), m, 256), ("deep_4096_n128", deep(users, 128, "deep128"), m, 128),
             ("batch_4096_n128", batch_4096_n128, m, 128), ("deep_262144_n256", deep(crowd, 256), many, 256)]
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), exclude_seen=True, loop_users=m, many_users=many),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0),
           "scratch_bytes": {str(n): int(sess.lib.poismf_hip_topn_deep_scratch_bytes(m, n, dimB, k)) for n in (128, 256, 1000)}}
    for name, _, nu, n in paths:
        out[name] = figure(ms[name], nu, n)
    out["speedup_deep_4096_n1000_over_loop"] = out["per_user_loop_n1000"]["ms"] / out["deep_4096_n1000"]["ms"]
    out["deep_over_batch_at_n128"] = out["deep_4096_n128"]["ms"] / out["batch_4096_n128"]["ms"]

    # the rows: both paths right under check_topn on sampled users; the two batched calls agree bit for bit at n = 128
    sample = np.sort(np.random.default_rng(2).choice(m, 16, replace=False))
    none = np.empty(0, np.uint64)
    for u in sample:
        for res in (keep["loop"], keep["deep1000"]):
            H.check_topn(A[u], B, res[0][u], res[1][u], none, rows[u], 1000, 1e-5)
    out["rows_with_identical_items_loop_vs_deep"] = int(np.all(keep["loop"][0] == keep["deep1000"][0], axis=1).sum())
    out["deep_equals_batch_at_n128"] = bool(np.array_equal(keep["deep128"][0], keep["batch128"][0])
                                            and keep["deep128"][1].tobytes() == keep["batch128"][1].tobytes())
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert out["deep_equals_batch_at_n128"]
    assert out["speedup_deep_4096_n1000_over_loop"] >= 10.0, out["speedup_deep_4096_n1000_over_loop"]


if __name__ == "__main__":
    main()
