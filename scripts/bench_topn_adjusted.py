#!/usr/bin/env python3
"""Time the batched top-N with per-(user, item) score factors (include/poismf_hip.h section 1r) against the exact route that exists
without it and against the plain call.

    python scripts/bench_topn_adjusted.py [--out profiles/topn_adjusted/bench_topn_adjusted.json] [--nnz 10000000] [--repeats 5]

scripts/bench_topn_weighted.py's workload and method: dimA 10^6, dimB 10^5, k = 50, fp32, random positive factors, a uniform CSR (synth),
n_top = 10, seen items excluded; a device-synchronised host clock around whole calls (the Python checks of the lists included), every
shape warmed up first, at least 0.5 s of timed work per figure, five repeats with the paths alternated inside each repeat; median, min
and max reported.  Every user lists --cells (100) cells, one drawn from each of as many equal strata of the items, with factors
log-uniform in [1/4, 4).

    adjusted_4096, adjusted_all   Session.topn_adjusted(exclude_seen=True) for the first 4096 users / all 10^6; with them the share of
                                  rows that differ from Session.topn_batch's
    route_4096, route_all         (a) the exact route without the call: Session.topn_batch(exclude_seen=True, exclude=cells) for the
                                  unlisted items, Session.topn_batch(include=cells, exclude_seen=True) to the depth of the row for the
                                  listed ones (possible only while a row has at most TOPN_BATCH_MAX_N_TOP cells), then the
                                  multiplication and the merge in numpy.  ASSERTED: items and score bits equal the call's on every row
    empty_4096, empty_all         (b) the call with nothing listed, next to plain_4096 / plain_all (Session.topn_batch on the same users
                                  in the same process): what the second stage's plumbing costs when it has nothing to do.  The rows
                                  are asserted equal; the ratio is recorded
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
from scripts.bench_topn_weighted import figure, timed


def host_merge(dense, listed, cells, factor, dimB, n_top):
    """route (a)'s host half: `dense` = (items, scores) [m x n_top] of the unlisted items, `listed` = (items, scores) [m x c] of the
    listed ones by plain score (TOPN_NONE pads a row the seen items shortened), cells / factor [m x c] the adjust rows, ascending.
    Every listed score times its cell's factor (one float multiplication), then every row's n_top best of both under (score
    descending, item ascending).  Returns (items, scores)."""
    l_ix, l_sc = listed
    m, c = cells.shape
    real = l_ix != api.TOPN_NONE
    key = (np.arange(m, dtype=np.int64)[:, None] * dimB + np.where(real, l_ix, 0).astype(np.int64)).reshape(-1)
    flat = (np.arange(m, dtype=np.int64)[:, None] * dimB + cells.astype(np.int64)).reshape(-1)       # ascending: rows in order, a row ascending
    pos = np.minimum(np.searchsorted(flat, key), flat.size - 1)
    f = factor.reshape(-1)[pos].reshape(m, c)
    a_sc = np.where(real, np.multiply(l_sc, f), -np.inf).astype(l_sc.dtype)
    ix = np.concatenate([dense[0], l_ix], axis=1)
    sc = np.concatenate([dense[1], a_sc], axis=1)
    by_item = np.argsort(ix, axis=1, kind="stable")                          # (TOPN_NONE is the largest index: the padding goes last)
    sc_i = np.take_along_axis(sc, by_item, 1)
    by_score = np.argsort(-sc_i, axis=1, kind="stable")[:, :n_top]           # (stable: ties stay in item order)
    pick = np.take_along_axis(by_item, by_score, 1)
    return np.take_along_axis(ix, pick, 1), np.take_along_axis(sc, pick, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_adjusted", "bench_topn_adjusted.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--cells", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-users", type=int, default=4096)
    args = ap.parse_args()
    dimA, dimB, k, n_top, m, c = args.dimA, args.dimB, args.k, 10, args.head_users, args.cells
    assert c <= api.TOPN_BATCH_MAX_N_TOP and dimB % c == 0, "route (a) lists a row's cells in one include call; the strata are equal"
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    everyone = np.arange(dimA, dtype=np.uint64)
    users = everyone[:m]
    width = dimB // c
    cells = (np.arange(c, dtype=np.uint64)[None, :] * np.uint64(width) + rng.integers(0, width, (dimA, c), dtype=np.uint64))   # a row ascending
    factor = np.exp(rng.uniform(np.log(0.25), np.log(4.0), (dimA, c))).astype(np.float32)
    indptr = np.arange(dimA + 1, dtype=np.uint64) * np.uint64(c)
    lists = {"4096": (users, (indptr[:m + 1], cells[:m].reshape(-1), factor[:m].reshape(-1))),
             "all": (everyone, (indptr, cells.reshape(-1), factor.reshape(-1)))}
    res = {}

    def adjusted(size):
        who, triple = lists[size]
        res[f"adjusted_{size}"] = sess.topn_adjusted(who, n_top, adjust=triple, exclude_seen=True, output_score=True)

    def route(size):
        who, triple = lists[size]
        pair = triple[:2]
        dense = sess.topn_batch(who, n_top, exclude_seen=True, exclude=pair, output_score=True)
        listed = sess.topn_batch(who, c, exclude_seen=True, include=pair, output_score=True)
        res[f"route_{size}"] = host_merge(dense, listed, cells[:len(who)], factor[:len(who)], dimB, n_top)

    def empty(size):
        res[f"empty_{size}"] = sess.topn_adjusted(lists[size][0], n_top, adjust=None, exclude_seen=True, output_score=True)

    def plain(size):
        res[f"plain_{size}"] = sess.topn_batch(lists[size][0], n_top, exclude_seen=True, output_score=True)

    paths = [(f"{name}_{size}", (lambda fn=fn, size=size: fn(size)), len(lists[size][0]))
             for size in ("4096", "all") for name, fn in (("adjusted", adjusted), ("route", route), ("empty", empty), ("plain", plain))]
    for name, fn, _ in paths:   # warm-up of every shape
        fn()
        print(f"warmed up {name}", file=sys.stderr, flush=True)
    ms = {name: [] for name, _, _ in paths}
    for rep in range(args.repeats):
        for name, fn, _ in paths:
            ms[name].append(timed(fn))
            print(f"repeat {rep} {name}: {ms[name][-1]:.1f} ms", file=sys.stderr, flush=True)
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, head_users=m, cells_per_user=c,
                            factor="log-uniform in [1/4, 4)"),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu in paths:
        out[name] = figure(ms[name], nu)
    same = lambda a, b: bool(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes())
    for size in ("4096", "all"):
        a, r, e, p = (res[f"{name}_{size}"] for name in ("adjusted", "route", "empty", "plain"))
        out[f"adjusted_{size}"]["share_of_rows_differing_from_topn_batch"] = float((a[0] != p[0]).any(axis=1).mean())
        out[f"route_{size}"]["rows_equal_adjusted_bits"] = same(r, a)
        out[f"empty_{size}"]["rows_equal_topn_batch"] = same(e, p)
        out[f"route_{size}"]["ms_over_adjusted_ms"] = out[f"route_{size}"]["ms"] / out[f"adjusted_{size}"]["ms"]
        out[f"adjusted_{size}"]["ms_over_topn_batch_ms"] = out[f"adjusted_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
        out[f"empty_{size}"]["ms_over_topn_batch_ms"] = out[f"empty_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    for size in ("4096", "all"):
        assert out[f"route_{size}"]["rows_equal_adjusted_bits"], f"the two routes differ on the {size} users"
        assert out[f"empty_{size}"]["rows_equal_topn_batch"], f"nothing listed differs from topn_batch on the {size} users"


if __name__ == "__main__":
    main()
