#!/usr/bin/env python3
"""Time the batched top-N (include/poismf_hip.h section 1f) against the per-user loop it replaces.

    python scripts/bench_topn.py [--out profiles/topn/bench_topn.json] [--nnz 10000000] [--repeats 5]
    python scripts/bench_topn.py --trace-pass        # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The metric's shape with random positive factors: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), n_top = 10, seen items
excluded.  Figures (each: a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of
timed work, five repeats, the paths alternated inside each repeat; median, min and max reported):

    per_user_loop   Session.topn(u, 10, exclude_ix = row u) over the first 4096 users -- the code that was there before
    batched_4096    the same users in one Session.topn_batch(exclude_seen=True) call
    batched_all     all 10^6 users in one call
    batched_4096_f64, host_pointers_4096 (poismf_hip_topn_batch: upload of B and of the users' rows of A included)

Next to each: users/s, the whole-call rate 2 users dimB k flop / time as a fraction of the fp32 (157.3) / fp64 (78.6) TFLOP/s
peak, and the floor max(flop / peak, bytes / 8 TB/s).  These are whole-call rates (uploads, merge and downloads included), not
the kernel's share of peak: that comes from the trace pass.  The condition the feature has to meet -- batched_4096 at least ten
times faster than per_user_loop in the same process, rows right under tests.helpers.check_topn -- is asserted.
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

PEAK = {True: 157.3e12, False: 78.6e12}
HBM = 8e12


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


def figure(ms_list, users, dimB, k, use_float, n_top):
    ms = float(np.median(ms_list))
    flop = 2.0 * users * dimB * k
    size = 4 if use_float else 8
    byts = (users * k + dimB * k) * size + users * n_top * (size + 4)   # each factor once, the results once
    floor_ms = max(flop / PEAK[use_float], byts / HBM) * 1e3
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3),
                whole_call_fraction_of_peak=flop / (ms * 1e-3) / PEAK[use_float], floor_ms=floor_ms, repeats=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn", "bench_topn.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=4096)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, n_top, m = args.dimA, args.dimB, args.k, 10, args.loop_users
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    users = np.arange(m, dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)

    if args.trace_pass:
        for _ in range(2):
            sess.topn_batch(users, n_top, exclude_seen=True, output_score=True)
            sess.topn_batch(everyone, n_top, exclude_seen=True, output_score=True)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 2}))
        return

    head = trip.row < m
    X = sp.csr_matrix((np.ones(int(head.sum()), np.float32), (trip.row[head], trip.col[head])), shape=(m, dimB))
    X.sum_duplicates(); X.sort_indices()
    rows = [X.indices[X.indptr[u]:X.indptr[u + 1]].astype(np.uint64) for u in range(m)]
    del trip

    loop_out = {}

    def per_user_loop():
        ix = np.empty((m, n_top), np.uint64)
        sc = np.empty((m, n_top), np.float32)
        for u in range(m):
            ix[u], sc[u] = sess.topn(u, n_top, exclude_ix=rows[u], output_score=True)
        loop_out["ix"], loop_out["sc"] = ix, sc

    bat_out = {}

    def batched_4096():
        bat_out["ix"], bat_out["sc"] = sess.topn_batch(users, n_top, exclude_seen=True, output_score=True)

    def batched_all():
        sess.topn_batch(everyone, n_top, exclude_seen=True, output_score=True)

    model = api.PoisMF(k=k, use_float=True)
    model.A, model.B, model.nusers, model.nitems, model.is_fitted = A, B, dimA, dimB, True
    host_out = {}

    def host_pointers_4096():
        host_out["ix"], host_out["sc"] = model.topN_batch(users, n_top, exclude=X, output_score=True)

    sess64 = api.Session.from_coo(sp.coo_matrix(X, shape=(m, dimB)), k, False)
    sess64.set_factors(A[:m].astype(np.float64), B.astype(np.float64))

    def batched_4096_f64():
        sess64.topn_batch(users, n_top, exclude_seen=True, output_score=True)

    paths = [("per_user_loop", per_user_loop, m, True), ("batched_4096", batched_4096, m, True), ("batched_all", batched_all, dimA, True),
             ("batched_4096_f64", batched_4096_f64, m, False), ("host_pointers_4096", host_pointers_4096, m, True)]
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, loop_users=m),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu, fl in paths:
        out[name] = figure(ms[name], nu, dimB, k, fl, n_top)
    out["speedup_batched_4096_over_loop"] = out["per_user_loop"]["ms"] / out["batched_4096"]["ms"]

    # the rows: both paths right under check_topn on sampled users; how many rows of the 4096 are identical is reported
    sample = np.sort(np.random.default_rng(2).choice(m, 64, replace=False))
    none = np.empty(0, np.uint64)
    for u in sample:
        for res in (loop_out, bat_out, host_out):
            H.check_topn(A[u], B, res["ix"][u], res["sc"][u], none, rows[u], n_top, 1e-5)
    out["rows_with_identical_items_loop_vs_batch"] = int(np.all(loop_out["ix"] == bat_out["ix"], axis=1).sum())
    out["host_pointer_rows_equal_session_rows"] = bool(np.array_equal(host_out["ix"], bat_out["ix"]) and np.array_equal(host_out["sc"], bat_out["sc"]))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    sess64.close()
    assert out["host_pointer_rows_equal_session_rows"]
    assert out["speedup_batched_4096_over_loop"] >= 10.0, out["speedup_batched_4096_over_loop"]


if __name__ == "__main__":
    main()
