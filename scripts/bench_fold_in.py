#!/usr/bin/env python3
"""Time the fold-in of new users on a resident session (include/poismf_hip.h section 1m) against the two-call route it replaces.

    python scripts/bench_fold_in.py [--out profiles/fold_in/bench_fold_in.json] [--nnz 10000000] [--repeats 5]

The README's shape with random positive factors: dimA 10^6, dimB 10^5, k = 50, fp32, a uniform CSR (synth); 4096 and 65 536 new
users with 100 items each (drawn with replacement, repeats merged); n_top = 10, the users' own items excluded; PG and CG at the
defaults of harness.auto_defaults.  Figures (each: a device-synchronised host clock around ONE whole call, every shape warmed up
first, five repeats, the routes alternated inside each repeat; median, min and max reported):

    session_topn_new    Session.topn_new(X, ...) with Bsum / Amean passed in: rows up, solve, top-N, indices and scores back
    two_calls           PoisMF.transform(X) (a throw-away session and an upload of B per call, factors back to the host), then
                        PoisMF.topN_batch on those factors with exclude = X (poismf_hip_topn_batch: B up a second time, the factors a
                        first) -- the only route there was
    session_transform   Session.transform(X, ...) alone: what of session_topn_new is guest set-up, solve and the factors' download

No ratio is asserted: the file records what was measured, and that both routes list the same items with the same scores.
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

from poismf_amd import api, synth


def once(fn):
    """ms of one call of fn between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def figure(ms_list, users):
    ms = float(np.median(ms_list))
    return dict(ms=ms, ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), users_per_s=users / (ms * 1e-3), repeats=len(ms_list))


def new_users(m, dimB, per_user, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), per_user)
    X = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, rng.integers(0, dimB, len(rows)))), shape=(m, dimB))
    X.sum_duplicates(); X.sort_indices()
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_in", "bench_fold_in.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--new-users", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--items-per-user", type=int, default=100)
    args = ap.parse_args()
    dimA, dimB, k, n_top = args.dimA, args.dimB, args.k, 10
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    rng = np.random.default_rng(1)
    A = rng.random((dimA, k), dtype=np.float32)
    B = rng.random((dimB, k), dtype=np.float32)
    sess = api.Session.from_coo(trip, k, True)
    sess.set_factors(A, B)
    nnz = int(sess.nnz(1))
    del trip
    Bsum, Amean = B.sum(axis=0), A.mean(axis=0)

    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, n_top=n_top, nnz=nnz, items_per_new_user=args.items_per_user, exclude_own=True),
           "method": "host clock around one whole call between device synchronisations; shapes warmed up; routes alternated; median of repeats",
           "device": torch.cuda.get_device_name(0)}
    for method in ("pg", "cg"):
        model = api.PoisMF(k=k, method=method, use_float=True)
        model.A, model.B, model.nusers, model.nitems, model.Bsum, model.Amean, model.is_fitted = A, B, dimA, dimB, Bsum, Amean, True
        holder = api.PoisMF(k=k, use_float=True)
        holder.B, holder.nitems, holder.is_fitted = B, dimB, True
        par = sess.make_params(method, model.l2_reg_, 0.0, 1.0, model.initial_step, model.limit_step, model.maxupd_, False, model.reuse_prev)
        for m in args.new_users:
            X = new_users(m, dimB, args.items_per_user, seed=m)
            users = np.arange(m, dtype=np.uint64)
            res = {}

            def session_topn_new():
                res["s"] = sess.topn_new(X, par, model.niter_, top_n=n_top, output_score=True, Bsum=Bsum, Amean=Amean)

            def two_calls():
                holder.A, holder.nusers = model.transform(X), m
                res["t"] = holder.topN_batch(users, n_top, exclude=X, output_score=True)

            def session_transform():
                sess.transform(X, par, model.niter_, Bsum=Bsum, Amean=Amean)

            paths = [("session_topn_new", session_topn_new), ("two_calls", two_calls), ("session_transform", session_transform)]
            for _, fn in paths:
                fn()
            ms = {name: [] for name, _ in paths}
            for _ in range(args.repeats):
                for name, fn in paths:
                    ms[name].append(once(fn))
            entry = {name: figure(ms[name], m) for name, _ in paths}
            entry["new_users"], entry["nnz_new"] = m, int(X.nnz)
            entry["niter"], entry["maxupd"], entry["l2_reg"] = int(model.niter_), int(model.maxupd_), float(model.l2_reg_)
            entry["speedup_session_over_two_calls"] = entry["two_calls"]["ms"] / entry["session_topn_new"]["ms"]
            entry["same_items_and_scores"] = bool(np.array_equal(res["s"][0], res["t"][0]) and np.array_equal(res["s"][1], res["t"][1]))
            out[f"{method}_{m}"] = entry
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()
    assert all(v["same_items_and_scores"] for v in out.values() if isinstance(v, dict) and "same_items_and_scores" in v)


if __name__ == "__main__":
    main()
