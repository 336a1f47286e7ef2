#!/usr/bin/env python3
"""Time an update of a resident session (include/poismf_hip.h section 2b) against the rebuild it replaces.

    python scripts/bench_session_update.py [--out profiles/session_update/bench_session_update.json] [--nnz 100000000] [--repeats 5]
    python scripts/bench_session_update.py --adds-only     # for a kernel trace: the session and the updates, nothing else

The README's workload: 1 000 000 x 100 000, about 1e8 nonzeros (uniform triplets, synth), k = 50, fp32.  Two sizes of update D:
4096 users x 10 cells, and 10^6 cells anywhere.  Figures (each: a device-synchronised host clock around whole calls in one process,
every route warmed up once, medians of `repeats` runs; every run of route (a) merges a D of its own, so each inserts new cells):

    add        (a) Session.add(D) on the resident session
    rebuild    (b) the only route there was: close the session, Session.from_coo(X + D), set_factors.  The triplets of X + D are
               concatenated on the host BEFORE the clock starts, which favours this route
    rows_4096  half_sweep_rows(1, the 4096 users of the small D) next to the full half_sweep(1) of the same session (PG at its
               defaults; reported, not asserted: a call over listed rows is launch-bound by construction)

Asserts only that (a) is faster than (b) at both sizes; prints both times and their ratio.
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


def update_of(kind, dimA, dimB, seed):
    rng = np.random.default_rng(seed)
    if kind == "users_4096x10":
        row = np.repeat(rng.choice(dimA, size=4096, replace=False), 10).astype(np.int64)
    else:
        row = rng.integers(0, dimA, 10 ** 6, dtype=np.int64)
    col = rng.integers(0, dimB, len(row), dtype=np.int64)
    return synth.Triplets(row, col, np.ones(len(row)), (dimA, dimB))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_update", "bench_session_update.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adds-only", action="store_true")
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
    kinds = ("users_4096x10", "cells_1e6")
    if args.adds_only:
        for kind in kinds:
            for rep in range(2):
                nnz_before = int(sess.nnz(1))
                fresh = sess.add(update_of(kind, dimA, dimB, 100 + rep))
                print(f"{kind}: nnz {nnz_before} + {fresh} new cells")
        sess.close()
        return
    for kind in kinds:
        ms_add, new_cells = [], []
        for rep in range(args.repeats + 1):
            D = update_of(kind, dimA, dimB, 100 + rep)
            new_cells.append(0)

            def add():
                new_cells[-1] = sess.add(D)

            ms_add.append(once(add))
        entry = {"add": figure(ms_add[1:]), "triplets": int(len(D.row)), "new_cells_last": int(new_cells[-1]), "nnz_after": int(sess.nnz(1))}
        out[kind] = entry
    # PG at its defaults: the 4096 users of the small update next to the whole A half of the same session
    l2, maxupd, _ = harness.auto_defaults("pg", k)
    par = sess.make_params("pg", l2, maxupd=maxupd)
    cd = sess.cnst_div(l2, 1e-7)
    users = np.unique(update_of("users_4096x10", dimA, dimB, 100).row)
    ms_rows, ms_full = [], []
    for rep in range(args.repeats + 1):
        ms_full.append(once(lambda: sess.half_sweep(1, par, 1e-7, cd)))
        ms_rows.append(once(lambda: sess.half_sweep_rows(1, users, par, 1e-7, cd)))
    out["rows_4096"] = {"half_sweep_rows": figure(ms_rows[1:]), "half_sweep": figure(ms_full[1:]), "rows": int(len(users)), "method": "pg", "maxupd": int(maxupd)}
    # (b) the rebuild, on X + D concatenated beforehand
    for kind in kinds:
        D = update_of(kind, dimA, dimB, 100)
        both = synth.Triplets(np.concatenate([trip.row, D.row]), np.concatenate([trip.col, D.col]),
                              np.concatenate([val32, D.data.astype(np.float32)]), (dimA, dimB))
        ms_rebuild = []
        holder = {"s": sess}

        def rebuild():
            holder["s"].close()
            holder["s"] = api.Session.from_coo(both, k, True)
            holder["s"].set_factors(A, B)

        for rep in range(args.repeats + 1):
            ms_rebuild.append(once(rebuild))
        sess = holder["s"]
        out[kind]["rebuild"] = figure(ms_rebuild[1:])
        out[kind]["rebuild_over_add"] = out[kind]["rebuild"]["ms"] / out[kind]["add"]["ms"]
        print(f"{kind}: add {out[kind]['add']['ms']:.3f} ms, rebuild {out[kind]['rebuild']['ms']:.3f} ms, ratio {out[kind]['rebuild_over_add']:.1f}")
        del both
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    for kind in kinds:
        assert out[kind]["add"]["ms"] < out[kind]["rebuild"]["ms"], (kind, out[kind])


if __name__ == "__main__":
    main()
