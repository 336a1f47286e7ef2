#!/usr/bin/env python3
"""Time the batched re-rank (include/poismf_hip.h section 1s) against the route it replaces and against the page call.

    python scripts/bench_order_include.py [--out profiles/order_include/bench.json] [--repeats 5]
    python scripts/bench_order_include.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The workload of scripts/bench_topn_include.py: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth), random positive factors,
uniformly drawn candidates; no exclusions, so that both routes do the same work.  Method as there: a device-synchronised host clock
around whole calls, every shape warmed up first, at least 0.5 s of timed work per figure, five repeats with the paths alternated
inside each repeat; median (min .. max).

    order_4096x100 / x1000 / x10000   Session.order_candidates(users, lists, output_score=True)
    order_all_x100                    all 10^6 users, 100 candidates each
    host_4096x100 / x1000 / x10000    Session.predict on every (user, candidate) pair, then np.lexsort((item, -score)) per user on the host
    host_65536x100                    the same for the first 65 536 users of the 10^6 (the per-user host loop over all of them is not run)
    page_4096x100 / x1000 / x10000    Session.topn_batch(users, 128, include=lists, output_score=True) on the same lists

Asserted at the three 4096-user shapes: both routes give identical items and score bits.  No speed-up is asserted.
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
from scripts.bench_topn_include import draw_lists, stat, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_include", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, m = args.dimA, args.dimB, args.k, 4096
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    del trip
    users = np.arange(m, dtype=np.uint64)
    lists = {ln: draw_lists(rng, dimB, [ln] * m) for ln in (100, 1000, 10000)}

    def order(u, incl):
        return sess.order_candidates(u, incl, output_score=True)

    if args.trace_pass:
        for _ in range(3):
            order(users, lists[1000])
            order(users, lists[10000])
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls_each": 3, "shapes": ["4096x1000", "4096x10000"]}))
        return

    def host(u, incl, ln):
        """the route before: the scores from the device, the order from np.lexsort per user (equal lengths: rows of a matrix)"""
        items = incl[1][:len(u) * ln]
        sc = sess.predict(np.repeat(u, ln), items).reshape(len(u), ln)
        it = items.reshape(len(u), ln)
        o = np.stack([np.lexsort((it[i], -sc[i].astype(np.float64))) for i in range(len(u))])
        return np.take_along_axis(it, o, 1), np.take_along_axis(sc, o, 1)

    everyone = np.arange(dimA, dtype=np.uint64)
    all100 = (np.arange(dimA + 1, dtype=np.uint64) * np.uint64(100),
              np.sort(rng.integers(0, dimB // 100, (dimA, 100)) + np.arange(100) * (dimB // 100), axis=1).astype(np.uint64).ravel())
    paths = [("order_all_x100", lambda: order(everyone, all100), dimA, 100 * dimA),
             ("host_65536x100", lambda: host(everyone[:65536], all100, 100), 65536, 100 * 65536)]
    for ln in (100, 1000, 10000):
        paths += [(f"order_4096x{ln}", lambda ln=ln: order(users, lists[ln]), m, ln * m),
                  (f"host_4096x{ln}", lambda ln=ln: host(users, lists[ln], ln), m, ln * m),
                  (f"page_4096x{ln}", lambda ln=ln: sess.topn_batch(users, 128, include=lists[ln], output_score=True), m, ln * m)]
    for _, fn, _, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), exclude_seen=False, users=m),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu, cells in paths:
        out[name] = stat(ms[name], nu, cells)
    same = {}
    for ln in (100, 1000, 10000):
        (_, ix, sc), (hix, hsc) = order(users, lists[ln]), host(users, lists[ln], ln)
        same[ln] = bool(np.array_equal(ix.reshape(m, ln), hix) and np.array_equal(sc.view(np.uint32).reshape(m, ln), hsc.view(np.uint32)))
        out[f"speedup_over_host_x{ln}"] = out[f"host_4096x{ln}"]["ms"] / out[f"order_4096x{ln}"]["ms"]
        out[f"over_page_x{ln}"] = out[f"order_4096x{ln}"]["ms"] / out[f"page_4096x{ln}"]["ms"]
    out["identical_items_and_score_bits"] = same
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert all(same.values()), same


if __name__ == "__main__":
    main()
