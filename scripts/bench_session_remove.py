#!/usr/bin/env python3
"""Time counts taken back from a resident session (include/poismf_hip.h section 2c) against the rebuild they replace.

    python scripts/bench_session_remove.py [--out profiles/session_remove/bench_session_remove.json] [--nnz 100000000] [--repeats 5]
    python scripts/bench_session_remove.py --calls-only     # for a kernel trace: the session and the three calls, nothing else

scripts/bench_session_update.py's resident matrix: 1 000 000 x 100 000, about 1e8 nonzeros (uniform triplets, synth), k = 50, fp32.
Three cases, each a visit of its own on stored cells no other visit names (the cells come from the session's own CSR, downloaded once):

    users_4096x10   Session.remove: 4096 users lose 10 stored cells each
    cells_1e6       Session.subtract: 10^6 stored cells anywhere are decremented, every second one to zero (it leaves), the others by half
    forget_4096     Session.forget(1, 4096 users)

Figures (each: a device-synchronised host clock around whole calls in one process, every route warmed up once, medians of `repeats` runs):

    call       (a) the call on the resident session
    rebuild    (b) the only route there was: close the session, Session.from_coo(X - D), set_factors.  The triplets of X - D are
               built on the host BEFORE the clock starts, which favours this route

Asserts that the range of (a)'s runs lies below the range of (b)'s runs in every case; prints medians, ranges and the ratio of the medians.
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

KINDS = ("users_4096x10", "cells_1e6", "forget_4096")
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


class Visits:
    """The cells of visit `rep` of each case, from the CSR (val, ind, ptr) the session holds at the start.  The users of the two per-user
    cases are drawn from the last tenth of the rows, no user twice; the decremented cells lie in the rows before, at evenly spread places
    of the CSR that differ from visit to visit."""

    def __init__(self, csr, dimA, dimB, visits, seed=7):
        self.val, self.ind, self.ptr = csr[0], csr[1], csr[2].astype(np.int64)
        self.shape = (dimA, dimB)
        cut = dimA - dimA // 10
        lens = np.diff(self.ptr)
        rich = cut + np.flatnonzero(lens[cut:] >= 10)
        users = np.random.default_rng(seed).permutation(rich)[:2 * visits * USERS]
        assert len(users) == 2 * visits * USERS, "too few users with 10 stored cells"
        self.users = users.reshape(2, visits, USERS)
        self.pool = int(self.ptr[cut])
        self.step = self.pool // 10 ** 6
        assert self.step >= visits, "too few stored cells for 10^6 distinct ones per visit"

    def places(self, kind, rep):
        """(places of the visit's cells in the CSR, its users or None)"""
        if kind == "cells_1e6":
            return np.arange(10 ** 6, dtype=np.int64) * self.step + rep, None
        users = self.users[0 if kind == "users_4096x10" else 1, rep]
        if kind == "forget_4096":
            return np.concatenate([np.arange(self.ptr[u], self.ptr[u + 1]) for u in users]), users
        return (self.ptr[users][:, None] + np.arange(10)[None, :]).ravel(), users

    def decrement(self, pos):
        """what cells_1e6 takes from the cells at `pos`: all of every second one, half of the others (exact in fp32)"""
        x = self.val[pos]
        return np.where(np.arange(len(pos)) % 2 == 0, x, x * np.float32(0.5)).astype(np.float32)

    def triplets(self, kind, rep):
        pos, _ = self.places(kind, rep)
        row = np.searchsorted(self.ptr, pos, side="right") - 1
        return synth.Triplets(row, self.ind[pos].astype(np.int64), self.decrement(pos) if kind == "cells_1e6" else np.ones(len(pos)), self.shape)

    def without(self, kind, rep):
        """(X - D of the visit as triplets: what the rebuild route is given, the cells that left)"""
        pos, _ = self.places(kind, rep)
        val = self.val.copy()
        val[pos] = val[pos] - self.decrement(pos) if kind == "cells_1e6" else 0
        keep = val > 0
        rows = np.repeat(np.arange(self.shape[0], dtype=np.int64), np.diff(self.ptr))
        return synth.Triplets(rows[keep], self.ind[keep].astype(np.int64), val[keep], self.shape), int(len(val) - keep.sum())


def call_of(sess, visits, kind, rep):
    if kind == "forget_4096":
        users = visits.places(kind, rep)[1]
        return lambda: sess.forget(1, users)
    D = visits.triplets(kind, rep)
    if kind == "cells_1e6":
        return lambda: sess.subtract(D)
    return lambda: sess.remove(D, missing="raise")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_remove", "bench_session_remove.json"))
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
    sess = api.Session.from_coo(trip, k, True)
    del trip
    sess.set_factors(A, B)
    n_visits = 2 if args.calls_only else args.repeats + 1
    visits = Visits(sess.matrix(1), dimA, dimB, n_visits)
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=int(sess.nnz(1)), precision="fp32"),
           "method": "host clock around whole calls between device synchronisations, one process; routes warmed up; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    if args.calls_only:
        for kind in KINDS:
            for rep in range(n_visits):
                nnz_before = int(sess.nnz(1))
                gone = call_of(sess, visits, kind, rep)()
                print(f"{kind}: nnz {nnz_before} - {gone} cells = {int(sess.nnz(1))}")
        sess.close()
        return
    for kind in KINDS:
        ms, gone = [], []
        for rep in range(n_visits):
            fn = call_of(sess, visits, kind, rep)
            gone.append(0)

            def call():
                gone[-1] = fn()

            ms.append(once(call))
        out[kind] = {"call": figure(ms[1:]), "cells_listed": int(len(visits.places(kind, n_visits - 1)[0])), "cells_removed_last": int(gone[-1]),
                     "nnz_after": int(sess.nnz(1))}
        assert sess.nnz(0) == sess.nnz(1)
    # (b) the rebuild, on X - D built beforehand from the matrix the session started with
    holder = {"s": sess}
    for kind in KINDS:
        less, n_gone = visits.without(kind, 0)

        def rebuild():
            holder["s"].close()
            holder["s"] = api.Session.from_coo(less, k, True)
            holder["s"].set_factors(A, B)

        ms = [once(rebuild) for rep in range(n_visits)]
        assert int(holder["s"].nnz(1)) == len(visits.val) - n_gone
        e = out[kind]
        e["rebuild"] = figure(ms[1:])
        e["rebuild_over_call"] = e["rebuild"]["ms"] / e["call"]["ms"]
        print(f"{kind}: call {e['call']['ms']:.3f} ms [{e['call']['ms_min']:.3f}, {e['call']['ms_max']:.3f}], rebuild {e['rebuild']['ms']:.3f} ms "
              f"[{e['rebuild']['ms_min']:.3f}, {e['rebuild']['ms_max']:.3f}], ratio {e['rebuild_over_call']:.1f}")
        del less
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
