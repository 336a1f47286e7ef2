#!/usr/bin/env python3
"""Time the batched ranks among candidate lists shared between users (include/poismf_hip.h section 1k) against its yardsticks.

    python scripts/bench_rank_shared.py [--out profiles/rank_shared/bench.json] [--repeats 5]
    python scripts/bench_rank_shared.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_rank_include.py: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), seen items excluded, random
positive factors, ten held-out cells per user; the pools are uniformly sampled and passed as they are (the united mode).  Method as
there: a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of timed work per figure,
five repeats with the paths alternated inside each repeat; median (min .. max).

    shared_4096x1000 / 8x1000 / x10000   Session.rank_batch(users, held_out, exclude_seen=True, include=table, include_of=, unite_test=True)
    shared_all_x100 / all_x10000         all 10^6 users on one pool
    include_*                            (a) Session.rank_batch(include=) with the pool written out per user and the held-out rows united in
                                         on the host (the lists are built before the clock starts); all 10^6 users x 10 000 is left out:
                                         its 10^10 indices cannot be held
    topn_*                               (b) Session.topn_batch(users, 10, include=table, include_of=) on the same table
    dense_4096x1000                      (c) Session.rank_batch(exclude=complement of pool and held-out row)

All three yardsticks run code this path does not touch.  Asserted at 4096 users x one pool of 1000: the new call gives (a)'s ranks and
is faster than (a) by more than the two paths' max - min spreads added together."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from poismf_amd import api, synth
from scripts.bench_topn_include import complement, draw_lists, stat, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_shared", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--no-include-all", action="store_true", help="leave out yardstick (a) for all users x 100 (800 MB of host lists)")
    args = ap.parse_args()
    dimA, dimB, k, m, per_user = args.dimA, args.dimB, args.k, 4096, 10
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

    # ten held-out cells per user: one from each tenth of the catalogue, ascending
    def held_out(n):
        step = dimB // per_user
        return (np.arange(n + 1, dtype=np.uint64) * np.uint64(per_user),
                (rng.integers(0, step, (n, per_user)) + np.arange(per_user) * step).astype(np.uint64).ravel())

    held = held_out(m)
    held_all = held_out(dimA)
    pool = {ln: draw_lists(rng, dimB, [ln]) for ln in (100, 1000, 10000)}
    pool8 = draw_lists(rng, dimB, [1000] * 8)
    of8 = rng.integers(0, 8, m).astype(np.uint64)

    def written(table, of, n, t):
        """every user's pool written out, its held-out row united in: what section 1j takes"""
        tp, ti = table[0].astype(np.int64), table[1]
        ln = np.diff(tp)[of]
        at = np.repeat(tp[:-1][of] - np.concatenate(([0], np.cumsum(ln)[:-1])), ln) + np.arange(int(ln.sum()))
        ip = np.zeros(n + 1, np.uint64)
        ip[1:] = np.cumsum(ln)
        return api._unite_rows((ip, ti[at]), t)

    def shared(u, t, table, of):
        return sess.rank_batch(u, t, exclude_seen=True, include=table, include_of=of, unite_test=True)

    def include(u, t, incl):
        return sess.rank_batch(u, t, exclude_seen=True, include=incl)

    def topn(u, table, of):
        return sess.topn_batch(u, 10, exclude_seen=True, include=table, include_of=of)

    if args.trace_pass:
        for _ in range(3):
            shared(users, held, pool[1000], 0)
            topn(users, pool[1000], 0)
            shared(users, held, pool[10000], 0)
            shared(everyone, held_all, pool[100], 0)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3,
                          "shapes": ["shared 4096x1000", "topn 4096x1000", "shared 4096x10000", "shared all x100"]}))
        return

    zeros = np.zeros(m, np.int64)
    w1000, w8, w10000 = written(pool[1000], zeros, m, held), written(pool8, of8.astype(np.int64), m, held), written(pool[10000], zeros, m, held)
    keep = {}
    comp = complement(w1000, m, dimB)

    def include_1000():
        keep["include"] = include(users, held, w1000)

    def dense():
        keep["dense"] = sess.rank_batch(users, held, exclude_seen=True, exclude=comp)

    cells = lambda table, n: int(np.diff(table[0].astype(np.int64)).max()) * n
    paths = [("shared_4096x1000", lambda: shared(users, held, pool[1000], 0), m, cells(pool[1000], m)),
             ("include_4096x1000", include_1000, m, cells(pool[1000], m)),
             ("topn_4096x1000", lambda: topn(users, pool[1000], 0), m, cells(pool[1000], m)),
             ("dense_4096x1000", dense, m, cells(pool[1000], m)),
             ("shared_4096x8x1000", lambda: shared(users, held, pool8, of8), m, cells(pool8, m)),
             ("include_4096x8x1000", lambda: include(users, held, w8), m, cells(pool8, m)),
             ("topn_4096x8x1000", lambda: topn(users, pool8, of8), m, cells(pool8, m)),
             ("shared_4096x10000", lambda: shared(users, held, pool[10000], 0), m, cells(pool[10000], m)),
             ("include_4096x10000", lambda: include(users, held, w10000), m, cells(pool[10000], m)),
             ("topn_4096x10000", lambda: topn(users, pool[10000], 0), m, cells(pool[10000], m)),
             ("shared_all_x100", lambda: shared(everyone, held_all, pool[100], 0), dimA, cells(pool[100], dimA)),
             ("topn_all_x100", lambda: topn(everyone, pool[100], 0), dimA, cells(pool[100], dimA)),
             ("shared_all_x10000", lambda: shared(everyone, held_all, pool[10000], 0), dimA, cells(pool[10000], dimA)),
             ("topn_all_x10000", lambda: topn(everyone, pool[10000], 0), dimA, cells(pool[10000], dimA))]
    if not args.no_include_all:
        w_all = written(pool[100], np.zeros(dimA, np.int64), dimA, held_all)
        paths.append(("include_all_x100", lambda: include(everyone, held_all, w_all), dimA, cells(pool[100], dimA)))

    print("inputs ready", file=sys.stderr, flush=True)
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name, _, _, _ in paths}
    for r in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
        print(f"repeat {r + 1} of {args.repeats} done", file=sys.stderr, flush=True)
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), exclude_seen=True, unite_test=True, users=m,
                            held_out_per_user=per_user),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0),
           "left_out": "include_all_x10000: 10^10 indices cannot be held" + ("; include_all_x100 by --no-include-all" if args.no_include_all else "")}
    for name, _, nu, nc in paths:
        out[name] = stat(ms[name], nu, nc)
    for shape in ("4096x1000", "4096x8x1000", "4096x10000", "all_x100", "all_x10000"):
        out[f"shared_over_topn_{shape}"] = out[f"shared_{shape}"]["ms"] / out[f"topn_{shape}"]["ms"]
        if f"include_{shape}" in out:
            out[f"include_over_shared_{shape}"] = out[f"include_{shape}"]["ms"] / out[f"shared_{shape}"]["ms"]
    out["dense_over_shared_4096x1000"] = out["dense_4096x1000"]["ms"] / out["shared_4096x1000"]["ms"]
    new, a = out["shared_4096x1000"], out["include_4096x1000"]
    got = shared(users, held, pool[1000], 0)
    out["ranks_equal_include"] = bool(np.array_equal(got[0], keep["include"][0]) and np.array_equal(got[1], keep["include"][1]))
    out["ranks_equal_dense"] = bool(np.array_equal(got[0], keep["dense"][0]) and np.array_equal(got[1], keep["dense"][1]))
    out["margin_over_include_ms"] = a["ms"] - new["ms"]
    out["summed_spreads_include_ms"] = (a["ms_max"] - a["ms_min"]) + (new["ms_max"] - new["ms_min"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert out["ranks_equal_include"] and out["ranks_equal_dense"]
    assert out["margin_over_include_ms"] > out["summed_spreads_include_ms"], (out["margin_over_include_ms"], out["summed_spreads_include_ms"])


if __name__ == "__main__":
    main()
