#!/usr/bin/env python3
"""Time the batched top-N over candidate lists shared between users (include/poismf_hip.h section 1i) against section 1h's call with
every user's list written out, and at one shape against the dense call with the complement as `exclude`.

    python scripts/bench_topn_shared.py [--out profiles/topn_shared/bench.json] [--repeats 5]
    python scripts/bench_topn_shared.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

DESIGN.md 4.11's workload: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), n_top = 10, seen items excluded, random positive
factors.  Method as in scripts/bench_topn_include.py: a device-synchronised host clock around whole calls, every shape warmed up first,
at least 0.5 s of timed work per figure, five repeats with the paths alternated inside each repeat; median (min .. max).

    shared_4096x1000 / include_4096x1000        4096 users on ONE list of 1000 candidates; the same list written out 4096 times
    shared_4096x8x1000 / include_4096x8x1000    the users spread over 8 lists of 1000
    shared_4096x10000 / include_4096x10000      one list of 10 000
    shared_all_x100 / include_all_x100          all 10^6 users on one list of 100
    shared_all_x10000                           all 10^6 users on one list of 10 000 (written out that is 10^10 indices, 80 GB of
                                                sparse_ix: section 1h's side of this figure cannot be built and is not measured)
    dense_4096x1000                             Session.topn_batch(users, 10, exclude_seen=True, exclude=complement of the list)

Recorded next to the times: whether the rows of the two paths are equal (items and scores, np.array_equal).  Asserted: at 4096 x 1000 on
one list and at 10^6 x 100 the shared call's median is below the include call's by more than the sum of the two paths' max - min spreads.
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


def draw(rng, dimB, ln):
    return np.sort(rng.choice(dimB, ln, replace=False)).astype(np.uint64)


def table_of(rows):
    indptr = np.zeros(len(rows) + 1, np.uint64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows)


def written_out(rows, of):
    """section 1h's argument: row of[i] of the table for every user i (equal lengths)"""
    ln = len(rows[0])
    return np.arange(len(of) + 1, dtype=np.uint64) * np.uint64(ln), np.stack(rows)[of].reshape(-1)


def stat(ms_list, users, cells):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3),
                ns_per_candidate=ms * 1e6 / max(cells, 1), repeats=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_shared", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
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

    one1000, one10000, one100 = [draw(rng, dimB, 1000)], [draw(rng, dimB, 10000)], [draw(rng, dimB, 100)]
    eight = [draw(rng, dimB, 1000) for _ in range(8)]
    of8 = rng.integers(0, 8, m)
    zeros_m, zeros_all = np.zeros(m, np.int64), np.zeros(dimA, np.int64)

    def shared(u, rows, of):
        return sess.topn_batch(u, n_top, exclude_seen=True, include=table_of(rows), include_of=of, output_score=True)

    def include(u, incl):
        return sess.topn_batch(u, n_top, exclude_seen=True, include=incl, output_score=True)

    if args.trace_pass:
        for _ in range(3):
            shared(users, one1000, zeros_m)
            shared(users, one10000, zeros_m)
            shared(everyone, one100, zeros_all)
            shared(everyone, one10000, zeros_all)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": ["4096x1000", "4096x10000", "1000000x100", "1000000x10000"]}))
        return

    inc = {"4096x1000": written_out(one1000, zeros_m), "4096x8x1000": written_out(eight, of8), "4096x10000": written_out(one10000, zeros_m),
           "all_x100": written_out(one100, zeros_all)}
    comp_row = np.setdiff1d(np.arange(dimB, dtype=np.uint64), one1000[0])
    comp = (np.arange(m + 1, dtype=np.uint64) * np.uint64(len(comp_row)), np.tile(comp_row, m))
    keep = {}

    def dense():
        keep["dense"] = sess.topn_batch(users, n_top, exclude_seen=True, exclude=comp, output_score=True)

    shapes = [("4096x1000", users, one1000, zeros_m), ("4096x8x1000", users, eight, of8), ("4096x10000", users, one10000, zeros_m),
              ("all_x100", everyone, one100, zeros_all)]
    paths = []
    for name, u, rows, of in shapes:
        cells = len(u) * len(rows[0])
        paths.append(("shared_" + name, lambda u=u, rows=rows, of=of: shared(u, rows, of), len(u), cells))
        paths.append(("include_" + name, lambda u=u, name=name: include(u, inc[name]), len(u), cells))
    paths.append(("shared_all_x10000", lambda: shared(everyone, one10000, zeros_all), dimA, dimA * 10000))
    paths.append(("dense_4096x1000", dense, m, 1000 * m))

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
    for name, u, rows, of in shapes:
        a, b = shared(u, rows, of), include(u, inc[name])
        new, old = out["shared_" + name], out["include_" + name]
        out["compare_" + name] = dict(rows_equal=bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])),
                                      include_over_shared=old["ms"] / new["ms"], margin_ms=old["ms"] - new["ms"],
                                      spreads_ms=(old["ms_max"] - old["ms_min"]) + (new["ms_max"] - new["ms_min"]))
        if name == "4096x1000":
            out["compare_dense_4096x1000"] = dict(rows_equal=bool(np.array_equal(a[0], keep["dense"][0]) and np.array_equal(a[1], keep["dense"][1])),
                                                  dense_over_shared=out["dense_4096x1000"]["ms"] / new["ms"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    for name, _, _, _ in shapes:
        assert out["compare_" + name]["rows_equal"], name
    assert out["compare_dense_4096x1000"]["rows_equal"]
    for name in ("4096x1000", "all_x100"):
        c = out["compare_" + name]
        assert c["margin_ms"] > c["spreads_ms"], (name, c)


if __name__ == "__main__":
    main()
