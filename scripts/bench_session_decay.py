#!/usr/bin/env python3
"""Time Session.decay on a resident session (include/poismf_hip.h section 2e) against the only exact route there was.

    python scripts/bench_session_decay.py [--out profiles/session_decay/bench_session_decay.json] [--nnz 100000000] [--repeats 5]
    python scripts/bench_session_decay.py --calls-only     # for a kernel trace: the session and the four calls, nothing else

scripts/bench_session_remove.py's resident matrix: 1 000 000 x 100 000, about 1e8 nonzeros (uniform triplets, synth: integer counts, 63 % of
them 1), k = 50, fp32.  Four cases, each ONE visit repeated on the matrix the session started with (put back before every run, outside the clock):

    inplace         decay(0.9): nothing leaves, the in-place pass
    half            decay(0.5, floor=0.75): the cells holding 1 leave (the counts are integers: no floor takes exactly half)
    half_vectors    decay(0.5, floor=f, users=U, items=I), U and I uniform in (0.5, 1.5), f the median of the scaled values: half leave
    zero_users      decay(1.0, users=0 on 4096 users, 1 elsewhere), next to forget(1, those users)

Figures (each: a device-synchronised host clock around whole calls in one process, every route warmed up once, medians of `repeats` runs):

    call       (a) the call on the resident session
    rebuild    (b) matrix(1) downloaded, scaled in numpy in the same operation order (the row of every entry expanded from the row pointers:
               the route needs triplets), close, Session.from_coo, set_factors

Asserts that both routes end with identical matrices in both orientations and that the range of (a)'s runs lies below the range of (b)'s
runs in every case; prints medians, ranges and the ratio of the medians.
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

KINDS = ("inplace", "half", "half_vectors", "zero_users")
USERS = 4096


def once(fn):
    """ms of one call of fn between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def figure(ms_list):
    return dict(ms=float(np.median(ms_list)), ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), repeats=len(ms_list))


def scaled(val, rows, ind, gamma, users, items):
    """((x * gamma) * users[row]) * items[col] in float32, one numpy operation per multiplication"""
    nv = val * np.float32(gamma)
    if users is not None:
        nv = nv * users[rows]
    if items is not None:
        nv = nv * items[ind]
    return nv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_decay", "bench_session_decay.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls-only", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k = args.dimA, args.dimB, args.k
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    holder = {"s": api.Session.from_coo(trip, k, True)}
    del trip
    holder["s"].set_factors(A, B)
    # the matrix every run starts from, as the triplets that put it back
    val0, ind0, ptr0 = holder["s"].matrix(1)
    rows0 = np.repeat(np.arange(dimA, dtype=np.int64), np.diff(ptr0.astype(np.int64)))
    start = synth.Triplets(rows0, ind0.astype(np.int64), val0, (dimA, dimB))
    nnz0 = len(val0)
    print(f"resident matrix: {nnz0} cells", flush=True)

    def restore():
        holder["s"].close()
        holder["s"] = api.Session.from_coo(start, k, True)
        holder["s"].set_factors(A, B)

    U, I = rng.uniform(0.5, 1.5, dimA).astype(np.float32), rng.uniform(0.5, 1.5, dimB).astype(np.float32)
    gone_users = rng.permutation(dimA)[:USERS]
    zeros = np.ones(dimA, np.float32)
    zeros[gone_users] = 0
    median = float(np.median(scaled(val0, rows0, start.col, 0.5, U, I)))
    cases = {"inplace": dict(gamma=0.9), "half": dict(gamma=0.5, floor=0.75), "half_vectors": dict(gamma=0.5, floor=median, users=U, items=I),
             "zero_users": dict(gamma=1.0, users=zeros)}
    if args.calls_only:
        for kind in KINDS:
            gone = holder["s"].decay(**cases[kind])
            print(f"{kind}: {gone} cells left the matrix, nnz {int(holder['s'].nnz(1))}", flush=True)
            restore()
        holder["s"].close()
        return
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=nnz0, precision="fp32"),
           "method": "host clock around whole calls between device synchronisations, one process; routes warmed up; median of repeats; "
                     "the session is put back to the starting matrix before every run, outside the clock",
           "device": torch.cuda.get_device_name(0)}
    for kind in KINDS:
        kw = cases[kind]
        gamma, floor, users, items = kw["gamma"], np.float32(kw.get("floor", 0.0)), kw.get("users"), kw.get("items")
        gone = [0]

        def call():
            gone[0] = holder["s"].decay(**kw)

        def rebuild():
            val, ind, ptr = holder["s"].matrix(1)
            rows = np.repeat(np.arange(dimA, dtype=np.int64), np.diff(ptr.astype(np.int64)))
            nv = scaled(val, rows, ind.astype(np.int64), gamma, users, items)
            keep = nv > floor
            less = synth.Triplets(rows[keep], ind[keep].astype(np.int64), nv[keep], (dimA, dimB))
            holder["s"].close()
            holder["s"] = api.Session.from_coo(less, k, True)
            holder["s"].set_factors(A, B)

        e = out[kind] = {}
        held = {}
        for route, fn in (("call", call), ("rebuild", rebuild)):
            ms = []
            for rep in range(args.repeats + 1):
                restore()
                ms.append(once(fn))
            e[route] = figure(ms[1:])
            held[route] = [holder["s"].matrix(w) for w in (1, 0)]
            print(f"{kind}: {route} {e[route]['ms']:.3f} ms [{e[route]['ms_min']:.3f}, {e[route]['ms_max']:.3f}]", flush=True)
        e["cells_removed"], e["nnz_after"] = int(gone[0]), len(held["call"][0][0])
        for a, b in zip(held["call"], held["rebuild"]):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), (kind, "the two routes hold different matrices")
        assert e["nnz_after"] == nnz0 - e["cells_removed"]
        del held
        if kind == "zero_users":
            ms = []
            for rep in range(args.repeats + 1):
                restore()
                ms.append(once(lambda: holder["s"].forget(1, gone_users)))
            e["forget"] = figure(ms[1:])
            print(f"{kind}: forget {e['forget']['ms']:.3f} ms [{e['forget']['ms_min']:.3f}, {e['forget']['ms_max']:.3f}]", flush=True)
        e["rebuild_over_call"] = e["rebuild"]["ms"] / e["call"]["ms"]
        print(f"{kind}: {e['cells_removed']} cells removed, ratio {e['rebuild_over_call']:.1f}", flush=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    holder["s"].close()
    for kind in KINDS:
        assert out[kind]["call"]["ms_max"] < out[kind]["rebuild"]["ms_min"], (kind, out[kind])


if __name__ == "__main__":
    main()
