#!/usr/bin/env python3
"""Time the batched top-N over include lists (include/poismf_hip.h section 1h) against the two ways there were before it.

    python scripts/bench_topn_include.py [--out profiles/topn_include/bench.json] [--repeats 5]
    python scripts/bench_topn_include.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing
    python scripts/bench_topn_include.py --new-only       # the new path's figures alone (comparing builds of the kernel)

DESIGN.md 4.11's workload: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), n_top = 10, seen items excluded, random positive
factors.  Method as in scripts/bench_topn.py: a device-synchronised host clock around whole calls, every shape warmed up first, at least
0.5 s of timed work per figure, five repeats with the paths alternated inside each repeat; median (min .. max).

    include_4096x100 / x1000 / x10000   Session.topn_batch(users, 10, exclude_seen=True, include=lists), uniformly drawn candidates
    include_all_x100                    all 10^6 users, 100 candidates each
    include_skew                        4096 users, log-uniform lengths 10 .. 50 000; include_equal is the same total in equal lengths
    loop_256x1000                       (a) Session.topn(u, 10, include_ix=list) one user at a time over the first 256 users, scaled to 4096
    dense_4096x1000                     (b) Session.topn_batch(users, 10, exclude_seen=True, exclude=complement of the list)

Asserted at 4096 users x 1000 candidates: the new call is faster than (a) and than (b), each by more than the larger max - min spread
of the two paths compared.  Also found: the list length at which (b) overtakes the new path for 4096 users (bisection).
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


def draw_lists(rng, dimB, lengths):
    """(indptr, indices) of uniformly drawn, sorted candidate lists (rejection of repeats per row)"""
    rows = []
    for ln in lengths:
        if ln >= dimB:
            r = np.arange(dimB)
        elif ln * 4 < dimB:
            r = np.unique(rng.integers(0, dimB, int(ln * 1.2) + 8))
            while len(r) < ln:
                r = np.unique(np.concatenate([r, rng.integers(0, dimB, ln)]))
            r = np.sort(rng.choice(r, ln, replace=False)) if len(r) > ln else r
        else:
            r = np.sort(rng.choice(dimB, ln, replace=False))
        rows.append(r)
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.uint64)


def complement(incl, m, dimB):
    """(indptr, indices) of every user's items outside its list"""
    mask = np.ones((m, dimB), bool)
    ip = incl[0].astype(np.int64)
    mask[np.repeat(np.arange(m), np.diff(ip)), incl[1].astype(np.int64)] = False
    indptr = np.zeros(m + 1, np.uint64)
    indptr[1:] = np.cumsum(mask.sum(axis=1))
    return indptr, np.nonzero(mask)[1].astype(np.uint64)


def stat(ms_list, users, cells):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3),
                ns_per_candidate=ms * 1e6 / max(cells, 1), repeats=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_include", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--new-only", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, n_top, m = args.dimA, args.dimB, args.k, 10, 4096
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    del trip
    users = np.arange(m, dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)

    lists = {ln: draw_lists(rng, dimB, [ln] * m) for ln in (100, 1000, 10000)}

    def include(u, incl):
        return sess.topn_batch(u, n_top, exclude_seen=True, include=incl, output_score=True)

    if args.trace_pass:
        for _ in range(3):
            include(users, lists[1000])
            include(users, lists[10000])
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": ["4096x1000", "4096x10000"]}))
        return

    skew_len = np.exp(rng.uniform(np.log(10), np.log(50000), m)).astype(np.int64)
    skew = draw_lists(rng, dimB, skew_len)
    equal_len = int(round(skew_len.sum() / m))
    equal = draw_lists(rng, dimB, [equal_len] * m)
    all100 = (np.arange(dimA + 1, dtype=np.uint64) * np.uint64(100),
              np.sort(rng.integers(0, dimB // 100, (dimA, 100)) + np.arange(100) * (dimB // 100), axis=1).astype(np.uint64).ravel())

    paths = [("include_4096x100", lambda: include(users, lists[100]), m, 100 * m),
             ("include_4096x1000", lambda: include(users, lists[1000]), m, 1000 * m),
             ("include_4096x10000", lambda: include(users, lists[10000]), m, 10000 * m),
             ("include_all_x100", lambda: include(everyone, all100), dimA, 100 * dimA),
             ("include_skew", lambda: include(users, skew), m, int(skew_len.sum())),
             ("include_equal", lambda: include(users, equal), m, equal_len * m)]
    keep = {}
    if not args.new_only:
        loop_m = 256
        loop_lists = [lists[1000][1][i * 1000:(i + 1) * 1000] for i in range(loop_m)]

        def loop():
            ix = np.empty((loop_m, n_top), np.uint64)
            for u in range(loop_m):
                ix[u], _ = sess.topn(u, n_top, include_ix=loop_lists[u], output_score=True)
            keep["loop"] = ix

        comp = complement(lists[1000], m, dimB)

        def dense():
            keep["dense"] = sess.topn_batch(users, n_top, exclude_seen=True, exclude=comp, output_score=True)

        paths += [("loop_256x1000", loop, loop_m, 1000 * loop_m), ("dense_4096x1000", dense, m, 1000 * m)]

    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, users=m),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu, cells in paths:
        out[name] = stat(ms[name], nu, cells)
    out["skew"] = dict(total_candidates=int(skew_len.sum()), longest=int(skew_len.max()), equal_length=equal_len,
                       skew_over_equal=out["include_skew"]["ns_per_candidate"] / out["include_equal"]["ns_per_candidate"])
    if not args.new_only:
        new = out["include_4096x1000"]
        a = dict(out["loop_256x1000"])
        for key in ("ms", "ms_min", "ms_max"):
            a[key] *= m / 256
        out["loop_scaled_to_4096"] = a
        b = out["dense_4096x1000"]
        got = include(users, lists[1000])
        out["rows_equal_dense"] = bool(np.array_equal(got[0], keep["dense"][0]) and np.array_equal(got[1], keep["dense"][1]))
        out["rows_with_identical_items_loop"] = int(np.all(keep["loop"] == got[0][:256], axis=1).sum())
        for other, name in ((a, "loop"), (b, "dense")):
            spread = max(other["ms_max"] - other["ms_min"], new["ms_max"] - new["ms_min"])
            out[f"margin_over_{name}_ms"] = other["ms"] - new["ms"]
            out[f"spread_{name}_ms"] = spread
            out[f"speedup_over_{name}"] = other["ms"] / new["ms"]
        # where the dense path overtakes: bisection over the list length (log scale), one timed figure per path and length
        lo, hi, steps = 1000, dimB, []
        full = draw_lists(rng, dimB, [dimB] * m)
        t_new, t_dense = timed(lambda: include(users, full)), timed(lambda: sess.topn_batch(users, n_top, exclude_seen=True, output_score=True))
        steps.append(dict(length=dimB, include_ms=t_new, dense_ms=t_dense))
        if t_dense < t_new:
            for _ in range(5):
                mid = int(round(np.sqrt(lo * hi) / 64) * 64)
                inc = draw_lists(rng, dimB, [mid] * m)
                cmp_ = complement(inc, m, dimB)
                include(users, inc)
                t_new = timed(lambda: include(users, inc))
                t_dense = timed(lambda: sess.topn_batch(users, n_top, exclude_seen=True, exclude=cmp_, output_score=True))
                steps.append(dict(length=mid, include_ms=t_new, dense_ms=t_dense))
                lo, hi = (lo, mid) if t_dense < t_new else (mid, hi)
            out["dense_overtakes_between"] = [lo, hi]
        else:
            out["dense_overtakes_between"] = None   # (not up to the whole catalogue)
        out["crossover_steps"] = steps
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    if not args.new_only:
        assert out["rows_equal_dense"]
        assert out["margin_over_loop_ms"] > out["spread_loop_ms"], (out["margin_over_loop_ms"], out["spread_loop_ms"])
        assert out["margin_over_dense_ms"] > out["spread_dense_ms"], (out["margin_over_dense_ms"], out["spread_dense_ms"])


if __name__ == "__main__":
    main()
