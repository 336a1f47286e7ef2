#!/usr/bin/env python3
"""Time the batched ranks among per-user include lists (include/poismf_hip.h section 1j) against its yardsticks.

    python scripts/bench_rank_include.py [--out profiles/rank_include/bench.json] [--repeats 5]
    python scripts/bench_rank_include.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

DESIGN.md 4.11's workload: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), seen items excluded, random positive factors, ten
held-out cells per user, united into lists of uniformly sampled negatives (so a list of "100 candidates" holds up to 110).  Method as in
scripts/bench_rank.py: a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of timed work per
figure, five repeats with the paths alternated inside each repeat; median (min .. max).

    rank_4096x100 / x1000 / x10000   Session.rank_batch(users, held_out, exclude_seen=True, include=lists)
    rank_all_x100                    all 10^6 users, 100 sampled negatives each
    rank_skew                        4096 users, log-uniform lengths 10 .. 50 000; rank_equal is the same total in equal lengths
    topn_*                           (a) Session.topn_batch(users, 10, exclude_seen=True, include=the same lists): the same gather
    dense_4096x1000                  (b) Session.rank_batch(users, held_out, exclude_seen=True, exclude=complement of the list)
    dense_all                        (c) Session.rank_batch over the whole catalogue for all 10^6 users: how evaluation is done without
                                     lists; reported for scale, not asserted

Asserted at 4096 users x 1000 candidates: the new call gives (b)'s ranks and is faster than (b) by more than the two paths' max - min
spreads added together."""
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
from scripts.bench_topn_include import complement, draw_lists, timed


def stat(ms_list, users, cells):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3),
                ns_per_candidate=ms * 1e6 / max(cells, 1), repeats=len(ms_list))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_include", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--no-dense-all", action="store_true", help="leave out yardstick (c), the slowest figure")
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
    lists = {ln: api._unite_rows(draw_lists(rng, dimB, [ln] * m), held) for ln in (100, 1000, 10000)}

    def rank(u, t, incl):
        return sess.rank_batch(u, t, exclude_seen=True, include=incl)

    def topn(u, incl):
        return sess.topn_batch(u, 10, exclude_seen=True, include=incl)

    if args.trace_pass:
        for _ in range(3):
            rank(users, held, lists[1000])
            topn(users, lists[1000])
            rank(users, held, lists[10000])
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": ["rank 4096x1000", "topn 4096x1000", "rank 4096x10000"]}))
        return

    skew_len = np.exp(rng.uniform(np.log(10), np.log(50000), m)).astype(np.int64)
    skew = api._unite_rows(draw_lists(rng, dimB, skew_len), held)
    equal_len = int(round(skew_len.sum() / m))
    equal = api._unite_rows(draw_lists(rng, dimB, [equal_len] * m), held)
    all100 = api._unite_rows((np.arange(dimA + 1, dtype=np.uint64) * np.uint64(100),
                              np.sort(rng.integers(0, dimB // 100, (dimA, 100)) + np.arange(100) * (dimB // 100), axis=1).astype(np.uint64).ravel()),
                             held_all)
    cells = lambda incl: int(incl[0][-1])
    keep = {}
    comp = complement(lists[1000], m, dimB)

    def dense():
        keep["dense"] = sess.rank_batch(users, held, exclude_seen=True, exclude=comp)

    paths = [("rank_4096x100", lambda: rank(users, held, lists[100]), m, cells(lists[100])),
             ("topn_4096x100", lambda: topn(users, lists[100]), m, cells(lists[100])),
             ("rank_4096x1000", lambda: rank(users, held, lists[1000]), m, cells(lists[1000])),
             ("topn_4096x1000", lambda: topn(users, lists[1000]), m, cells(lists[1000])),
             ("rank_4096x10000", lambda: rank(users, held, lists[10000]), m, cells(lists[10000])),
             ("topn_4096x10000", lambda: topn(users, lists[10000]), m, cells(lists[10000])),
             ("rank_all_x100", lambda: rank(everyone, held_all, all100), dimA, cells(all100)),
             ("topn_all_x100", lambda: topn(everyone, all100), dimA, cells(all100)),
             ("rank_skew", lambda: rank(users, held, skew), m, cells(skew)),
             ("rank_equal", lambda: rank(users, held, equal), m, cells(equal)),
             ("dense_4096x1000", dense, m, cells(lists[1000]))]
    if not args.no_dense_all:
        paths.append(("dense_all", lambda: sess.rank_batch(everyone, held_all, exclude_seen=True), dimA, dimA * dimB))

    print("inputs ready", file=sys.stderr, flush=True)
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name, _, _, _ in paths}
    for r in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
        print(f"repeat {r + 1} of {args.repeats} done", file=sys.stderr, flush=True)
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), exclude_seen=True, users=m, held_out_per_user=per_user),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu, nc in paths:
        out[name] = stat(ms[name], nu, nc)
    for shape in ("4096x100", "4096x1000", "4096x10000", "all_x100"):
        out[f"rank_over_topn_{shape}"] = out[f"rank_{shape}"]["ms"] / out[f"topn_{shape}"]["ms"]
    out["skew"] = dict(total_candidates=cells(skew), longest=int(np.diff(skew[0].astype(np.int64)).max()), equal_length=equal_len,
                       skew_over_equal=out["rank_skew"]["ns_per_candidate"] / out["rank_equal"]["ns_per_candidate"])
    new, b = out["rank_4096x1000"], out["dense_4096x1000"]
    got = rank(users, held, lists[1000])
    out["ranks_equal_dense"] = bool(np.array_equal(got[0], keep["dense"][0]) and np.array_equal(got[1], keep["dense"][1]))
    out["margin_over_dense_ms"] = b["ms"] - new["ms"]
    out["summed_spreads_dense_ms"] = (b["ms_max"] - b["ms_min"]) + (new["ms_max"] - new["ms_min"])
    out["speedup_over_dense"] = b["ms"] / new["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert out["ranks_equal_dense"]
    assert out["margin_over_dense_ms"] > out["summed_spreads_dense_ms"], (out["margin_over_dense_ms"], out["summed_spreads_dense_ms"])


if __name__ == "__main__":
    main()
