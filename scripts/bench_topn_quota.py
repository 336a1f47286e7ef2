#!/usr/bin/env python3
"""Time the batched top-N with per-group quotas (include/poismf_hip.h section 1n) against the plain call and against the route it
replaces.

    python scripts/bench_topn_quota.py [--out profiles/topn_quota/bench_topn_quota.json] [--nnz 10000000] [--repeats 5]

scripts/bench_topn.py's workload and method: dimA 10^6, dimB 10^5, k = 50, fp32, random positive factors, a uniform CSR (synth),
n_top = 10, seen items excluded; a device-synchronised host clock around whole calls, every shape warmed up first, at least 0.5 s of
timed work per figure, five repeats with the paths alternated inside each repeat; median, min and max reported.  1000 groups
(item j is in group j % 1000) at quota 2 -- lowered to 1, and said so in the output, if under 10 % of the rows would differ from the plain
call's.

    quota_4096, quota_all     Session.topn_quota(exclude_seen=True) for the first 4096 users / all 10^6; with them the share of rows that
                              differ from Session.topn_batch's (the quotas bind on this workload)
    loose_4096, loose_all     every quota = n_top, so nothing binds, next to plain_4096 / plain_all (Session.topn_batch on the same
                              users in the same process): the ratio is the price of the group-aware prune.  Recorded, not asserted
    deep_route_4096           today's only route: Session.topn_deep(users, 1000, exclude_seen=True) and a vectorised numpy walk of the
                              1000 entries per user on the host

Asserted: the deep route's rows equal quota_4096's wherever its 1000 entries yielded ten survivors, and quota_4096 is faster than it.
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


def figure(ms_list, users):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3), repeats=len(ms_list))


def host_walk(ix, sc, group_of, quota, n_top):
    """the quota rule applied on the host to ranked lists [m x depth] (TOPN_NONE pads a short one): every row's first n_top entries that
    have fewer than quota[g] entries of their group before them.  Returns (items, scores, rows that found n_top survivors)."""
    m, depth = ix.shape
    real = ix != api.TOPN_NONE
    g = np.where(real, group_of[np.where(real, ix, 0)], len(quota)).astype(np.int64)   # (the padding: a group of its own, quota 0)
    q = np.append(quota, 0)
    order = np.argsort(g, axis=1, kind="stable")
    gs = np.take_along_axis(g, order, 1)
    pos = np.broadcast_to(np.arange(depth), (m, depth))
    run = np.ones((m, depth), bool)
    run[:, 1:] = gs[:, 1:] != gs[:, :-1]
    rank_sorted = pos - np.maximum.accumulate(np.where(run, pos, 0), axis=1)
    rank = np.empty_like(rank_sorted)
    np.put_along_axis(rank, order, rank_sorted, 1)
    keep = rank < q[g]
    nth = np.cumsum(keep, axis=1)
    out_ix = np.full((m, n_top), api.TOPN_NONE, np.uint64)
    out_sc = np.full((m, n_top), -np.inf, sc.dtype)
    r, c = np.nonzero(keep & (nth <= n_top))
    out_ix[r, nth[r, c] - 1] = ix[r, c]
    out_sc[r, nth[r, c] - 1] = sc[r, c]
    return out_ix, out_sc, nth[:, -1] >= n_top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_quota", "bench_topn_quota.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head-users", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=1000)
    args = ap.parse_args()
    dimA, dimB, k, n_top, m, n_groups = args.dimA, args.dimB, args.k, 10, args.head_users, args.groups
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    users = np.arange(m, dtype=np.uint64)
    everyone = np.arange(dimA, dtype=np.uint64)
    group_of = (np.arange(dimB) % n_groups).astype(np.uint64)

    def quota_call(who, q):
        return sess.topn_quota(who, n_top, group_of=group_of, quota=q, exclude_seen=True, output_score=True)

    def plain_call(who):
        return sess.topn_batch(who, n_top, exclude_seen=True, output_score=True)

    # the quota the figures are taken at: 2, unless it changes fewer than one row in ten of the first 4096
    plain_head = plain_call(users)
    quota, tried = 2, {}
    for q in (2, 1):
        quota = q
        tried[q] = float((quota_call(users, q)[0] != plain_head[0]).any(axis=1).mean())
        if tried[q] >= 0.10:
            break
    qv = np.full(n_groups, quota, np.uint64)
    res = {}

    def quota_4096():
        res["quota_4096"] = quota_call(users, quota)

    def quota_all():
        res["quota_all"] = quota_call(everyone, quota)

    def loose_4096():
        res["loose_4096"] = quota_call(users, n_top)

    def loose_all():
        res["loose_all"] = quota_call(everyone, n_top)

    def plain_4096():
        res["plain_4096"] = plain_call(users)

    def plain_all():
        res["plain_all"] = plain_call(everyone)

    def deep_route_4096():
        ix, sc = sess.topn_deep(users, 1000, exclude_seen=True, output_score=True)
        res["deep_route_4096"] = host_walk(ix, sc, group_of, qv, n_top)

    paths = [("quota_4096", quota_4096, m), ("loose_4096", loose_4096, m), ("plain_4096", plain_4096, m), ("deep_route_4096", deep_route_4096, m),
             ("quota_all", quota_all, dimA), ("loose_all", loose_all, dimA), ("plain_all", plain_all, dimA)]
    for _, fn, _ in paths:   # warm-up of every shape
        fn()
    ms = {name: [] for name, _, _ in paths}
    for _ in range(args.repeats):
        for name, fn, _ in paths:
            ms[name].append(timed(fn))
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=int(sess.nnz(1)), exclude_seen=True, head_users=m, groups=n_groups,
                            group_of="j % groups", quota=quota, share_of_rows_changed_by_quota_tried={str(q): v for q, v in tried.items()}),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; paths alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for name, _, nu in paths:
        out[name] = figure(ms[name], nu)
    for size in ("4096", "all"):
        out[f"quota_{size}"]["share_of_rows_differing_from_topn_batch"] = float(
            (res[f"quota_{size}"][0] != res[f"plain_{size}"][0]).any(axis=1).mean())
        out[f"loose_{size}"]["ms_over_topn_batch_ms"] = out[f"loose_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
        out[f"quota_{size}"]["ms_over_topn_batch_ms"] = out[f"quota_{size}"]["ms"] / out[f"plain_{size}"]["ms"]
        out[f"loose_{size}"]["rows_equal_topn_batch"] = bool(np.array_equal(res[f"loose_{size}"][0], res[f"plain_{size}"][0]) and
                                                             res[f"loose_{size}"][1].tobytes() == res[f"plain_{size}"][1].tobytes())
    d_ix, d_sc, d_full = res["deep_route_4096"]
    q_ix, q_sc = res["quota_4096"]
    out["deep_route_4096"]["rows_with_ten_survivors"] = int(d_full.sum())
    out["deep_route_4096"]["rows_equal_quota_4096_where_ten_survived"] = bool(np.array_equal(d_ix[d_full], q_ix[d_full]) and
                                                                              d_sc[d_full].tobytes() == q_sc[d_full].tobytes())
    out["speedup_quota_4096_over_deep_route"] = out["deep_route_4096"]["ms"] / out["quota_4096"]["ms"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert out["loose_4096"]["rows_equal_topn_batch"] and out["loose_all"]["rows_equal_topn_batch"]
    assert out["deep_route_4096"]["rows_equal_quota_4096_where_ten_survived"]
    assert out["speedup_quota_4096_over_deep_route"] > 1.0, out["speedup_quota_4096_over_deep_route"]


if __name__ == "__main__":
    main()
