#!/usr/bin/env python3
"""Time explain (include/poismf_hip.h section 1v) against the only route there was before it: numpy on a host copy of the factors.

    python scripts/bench_explain.py [--out profiles/explain/bench.json] [--repeats 5] [--host-repeats-all 5]
    python scripts/bench_explain.py --trace-pass     # what to put under `rocprofv3 --kernel-trace --stats -- ...`: no timing

The README workload with seen rows of about 100: dimA 10^6, dimB 10^5, k 50, fp32, a uniform CSR (synth) of 10^8 cells, pages of
Session.topn_batch(top_n=10, exclude_seen=True), m = 5, comp_scale = 1 / (colsum(B) + 0.1).  A device-synchronised host clock around
whole calls, every shape warmed up first, at least 0.5 s of timed work per figure; median (min .. max).

    gpu_<shape>    Session.explain(users, pages, m=5, comp_scale=g)
    host_<shape>   per chunk of 2048 users: B[seen] gathered (padded to the chunk's longest row), one batched matmul against
                   [a | q_1 .. q_10], the division, a lexsort per cell -- all in float32 numpy
    shapes: 4096 users, all 10^6 users

Asserted: on the first 4096 users, both routes name the same items on every cell whose float64 contributions are further apart
than (2 k + 8) 2^-24 relative around the m-th place and within the first m (tests/test_gpu_explain.py's bound); the all-users run
reports the share of cells on which the float32 routes agree outright.  No ratio is asserted: the ratio is what this measures.
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
from scripts.bench_topn_include import stat, timed


def host_route(A, B, users, pages, indptr, indices, values, g, m, dt=np.float32, chunk=2048, want_values=False):
    """(items [n x q x m], and with want_values the sorted contributions [n x q x L] per chunk as a list) in `dt`"""
    out, vals = np.empty(pages.shape + (m,), np.int64), []
    A, B, g = A.astype(dt, copy=False), B.astype(dt, copy=False), g.astype(dt)
    for c0 in range(0, len(users), chunk):
        u = users[c0:c0 + chunk].astype(np.int64)
        lo, ln = indptr[u], indptr[u + 1] - indptr[u]
        L = max(int(ln.max()), m)
        pos = np.minimum(lo[:, None] + np.arange(L), len(indices) - 1)
        pad = np.arange(L)[None, :] >= ln[:, None]
        idx = np.where(pad, np.iinfo(np.int64).max, indices[pos])
        Bs = B[indices[pos]]                                                    # [c, L, k]
        cols = np.concatenate((A[u][:, None, :], (A[u] * g)[:, None, :] * B[pages[c0:c0 + chunk].astype(np.int64)]), axis=1)
        prod = np.matmul(Bs, cols.transpose(0, 2, 1))                          # [c, L, 1 + q]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = values[pos].astype(dt)[:, :, None] * prod[:, :, 1:] / prod[:, :, :1]
        v[~np.isfinite(v)] = 0
        v[np.broadcast_to(pad[:, :, None], v.shape)] = -np.inf
        order = np.lexsort((np.broadcast_to(idx[:, :, None], v.shape), -v), axis=1)
        out[c0:c0 + chunk] = np.take_along_axis(np.broadcast_to(idx[:, :, None], v.shape), order[:, :m, :], axis=1).transpose(0, 2, 1)
        if want_values:
            vals.append(np.take_along_axis(v, order, axis=1).transpose(0, 2, 1))
    return out, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats-all", type=int, default=5)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k, n, m = args.dimA, args.dimB, args.k, 10, 5
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    rng = np.random.default_rng(1)
    A, B = rng.random((dimA, k), dtype=np.float32), rng.random((dimB, k), dtype=np.float32)
    sess.set_factors(A, B)
    g = (1.0 / (B.sum(0, dtype=np.float64) + 0.1)).astype(np.float32)
    everyone, few = np.arange(dimA, dtype=np.uint64), min(4096, dimA)
    pages = sess.topn_batch(everyone, n, exclude_seen=True)[0]

    def gpu(nu):
        return sess.explain(everyone[:nu], pages[:nu], m=m, comp_scale=g)

    if args.trace_pass:
        for _ in range(3):
            gpu(few)
        torch.cuda.synchronize()
        sess.close()
        print(json.dumps({"trace_pass": True, "calls": 3, "users": few}))
        return

    values, indices, indptr = (np.asarray(v) for v in sess.matrix(1))
    indptr, indices = indptr.astype(np.int64), indices.astype(np.int64)

    def host(nu):
        return host_route(A, B, everyone[:nu], pages[:nu], indptr, indices, values, g, m)[0]

    # the assertion, on the first users: cells whose float64 contributions are clear of each other down to the m-th place
    ix_few = gpu(few)[0].astype(np.int64)
    host_few = host(few)
    _, v64 = host_route(A, B, everyone[:few], pages[:few], indptr, indices, values, g, m, np.float64, want_values=True)
    tol, clear = (2 * k + 8) * 2.0 ** -24, []
    for v in v64:
        top = v[:, :, :m + 1]
        with np.errstate(invalid="ignore"):
            clear.append(np.all(top[:, :, :-1] - top[:, :, 1:] > 2 * tol * np.abs(top[:, :, :-1]), axis=2))   # (a row shorter than m + 1: not clear)
    clear = np.concatenate(clear)
    agree_clear = bool(np.array_equal(ix_few[clear], host_few[clear]))

    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), page=n, m=m, precision="fp32"),
           "method": "host clock around whole calls between device synchronisations; >= 0.5 s per figure; median of repeats",
           "device": torch.cuda.get_device_name(0), "cells_clear_of_ties_4096": int(clear.sum()), "cells_4096": int(clear.size),
           "same_items_on_clear_cells_4096": agree_clear}
    for name, nu in (("4096", few), ("all", dimA)):
        gpu(nu)
        out["gpu_" + name] = stat([timed(lambda: gpu(nu)) for _ in range(args.repeats)], nu, nu * n)
        reps = args.repeats if nu == few else args.host_repeats_all
        if reps > 0:
            out["host_" + name] = stat([timed(lambda: host(nu)) for _ in range(reps)], nu, nu * n)
            out["host_over_gpu_" + name] = out["host_" + name]["ms"] / out["gpu_" + name]["ms"]
    if args.host_repeats_all > 0:
        out["share_of_cells_with_the_same_items_all"] = float(np.mean(np.all(gpu(dimA)[0].astype(np.int64) == host(dimA), axis=2)))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert agree_clear, "the two routes name different items on a cell without near-ties"


if __name__ == "__main__":
    main()
