#!/usr/bin/env python3
"""Time new rows joining a resident session (include/poismf_hip.h section 2d) against the rebuild they replace.

    python scripts/bench_session_append.py [--out profiles/session_append/bench_session_append.json] [--nnz 100000000] [--repeats 5]
    python scripts/bench_session_append.py --growth-only   # for a kernel trace: the session and appends of empty rows, nothing else

The README's workload: 1 000 000 x 100 000, about 1e8 nonzeros (uniform triplets, synth), k = 50, fp32.  Figures (each: a
device-synchronised host clock around whole calls in one process, every route warmed up once, medians of `repeats` runs; every run
appends rows of its own, so the session keeps growing while it is timed):

    growth_4096        Session.append(1, n_new=4096): no cells -- the growth kernels, the swap and the grown half's sort alone
    users_given        Session.append_users(4096 users x 10 cells, factors=given)
    users_adopted      Session.append_users(the same users) through transform and adopt_new (PG at its defaults, 3 iterations, Bsum and
                       Amean passed in); `transform` is the fold-in alone, timed next to it on the same rows
    items_1000x100     Session.append_items(1000 items x 100 cells, start=given): the append and the one local refit of the new rows
    rebuild            the only route there was, next to each: close the session, Session.from_coo(X grown), set_factors.  The triplets
                       of the grown matrix are concatenated on the host BEFORE the clock starts, which favours this route

Asserts only that each in-place route is faster than the rebuild measured beside it; prints the times and their ratios.
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

from poismf_amd import api, harness, synth


def once(fn):
    """ms of one call of fn between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def figure(ms_list):
    return dict(ms=float(np.median(ms_list)), ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), repeats=len(ms_list))


def rows_of(n, per_row, width, seed):
    """n new rows of per_row cells each over `width` columns, as a CSR matrix of ones (a repeated column inside a row is summed)"""
    rng = np.random.default_rng(seed)
    X = sp.csr_matrix((np.ones(n * per_row, np.float32), (np.repeat(np.arange(n), per_row), rng.integers(0, width, n * per_row))), shape=(n, width))
    X.sum_duplicates()
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_append", "bench_session_append.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--growth-only", action="store_true")
    args = ap.parse_args()
    dimA, dimB, k = args.dimA, args.dimB, args.k
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    val32 = trip.data.astype(np.float32)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), precision="fp32"),
           "method": "host clock around whole calls between device synchronisations, one process; routes warmed up; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    n_users, n_items = 4096, 1000
    if args.growth_only:
        for rep in range(3):
            first = sess.append(1, n_new=n_users)
            print(f"append(1, n_new={n_users}): users {first} .. {sess.dimA - 1}")
        sess.close()
        return
    l2, maxupd, _ = harness.auto_defaults("pg", k)
    par = sess.make_params("pg", l2, maxupd=maxupd)
    Bsum, Amean, start = B.sum(axis=0), A.mean(axis=0), B.mean(axis=0)
    F = rng.random((n_users, k), dtype=np.float32)
    reps = range(args.repeats + 1)

    ms = [once(lambda: sess.append(1, n_new=n_users)) for rep in reps]
    out["growth_4096"] = {"append": figure(ms[1:]), "rows": n_users, "dimA_after": sess.dimA}

    ms = []
    for rep in reps:
        X = rows_of(n_users, 10, dimB, 100 + rep)
        ms.append(once(lambda: sess.append_users(X, par, 3, factors=F)))
    out["users_given"] = {"append": figure(ms[1:]), "rows": n_users, "cells": int(X.nnz), "dimA_after": sess.dimA, "nnz_after": int(sess.nnz(1))}

    ms, ms_fold = [], []
    for rep in reps:
        X = rows_of(n_users, 10, dimB, 200 + rep)
        ms_fold.append(once(lambda: sess.transform(X, par, 3, Bsum=Bsum, Amean=Amean)))
        ms.append(once(lambda: sess.append_users(X, par, 3, Bsum=Bsum, Amean=Amean)))
    out["users_adopted"] = {"append": figure(ms[1:]), "transform": figure(ms_fold[1:]), "rows": n_users, "cells": int(X.nnz), "method": "pg",
                            "niter": 3, "dimA_after": sess.dimA, "nnz_after": int(sess.nnz(1))}

    ms = []
    for rep in reps:
        X = rows_of(n_items, 100, sess.dimA, 300 + rep)
        ms.append(once(lambda: sess.append_items(X, par, 1e-7, start=start)))
    out["items_1000x100"] = {"append": figure(ms[1:]), "rows": n_items, "cells": int(X.nnz), "method": "pg", "maxupd": int(maxupd),
                             "dimB_after": sess.dimB, "nnz_after": int(sess.nnz(1))}

    # the rebuild, on the grown matrix concatenated beforehand: X and 4096 users x 10 cells, X and 1000 items x 100 cells
    Xu, Xi = rows_of(n_users, 10, dimB, 100).tocoo(), rows_of(n_items, 100, dimA, 300).tocoo()
    grown = {
        "users": (synth.Triplets(np.concatenate([trip.row, dimA + Xu.row.astype(np.int64)]), np.concatenate([trip.col, Xu.col.astype(np.int64)]),
                                 np.concatenate([val32, Xu.data]), (dimA + n_users, dimB)), np.vstack([A, F]), B),
        "items": (synth.Triplets(np.concatenate([trip.row, Xi.col.astype(np.int64)]), np.concatenate([trip.col, dimB + Xi.row.astype(np.int64)]),
                                 np.concatenate([val32, Xi.data]), (dimA, dimB + n_items)), A, np.vstack([B, np.tile(start, (n_items, 1))])),
    }
    holder = {"s": sess}
    for what, (both, Ag, Bg) in grown.items():
        def rebuild():
            holder["s"].close()
            holder["s"] = api.Session.from_coo(both, k, True)
            holder["s"].set_factors(Ag, Bg)

        out["rebuild_" + what] = figure([once(rebuild) for rep in reps][1:])
    holder["s"].close()
    for kind, what in (("growth_4096", "users"), ("users_given", "users"), ("users_adopted", "users"), ("items_1000x100", "items")):
        out[kind]["rebuild"] = out["rebuild_" + what]
        out[kind]["rebuild_over_append"] = out[kind]["rebuild"]["ms"] / out[kind]["append"]["ms"]
        print(f"{kind}: in place {out[kind]['append']['ms']:.3f} ms, rebuild {out[kind]['rebuild']['ms']:.3f} ms, ratio {out[kind]['rebuild_over_append']:.1f}")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    for kind in ("growth_4096", "users_given", "users_adopted", "items_1000x100"):
        assert out[kind]["append"]["ms"] < out[kind]["rebuild"]["ms"], (kind, out[kind])


if __name__ == "__main__":
    main()
