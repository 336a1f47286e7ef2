#!/usr/bin/env python3
"""Time Session.holdout on a resident session (include/poismf_hip.h section 2f) against the only route there was.

    python scripts/bench_session_holdout.py [--out profiles/session_holdout/bench.json] [--nnz 100000000] [--repeats 5]
    python scripts/bench_session_holdout.py --calls-only     # for a kernel trace: the session and the three calls, nothing else

scripts/bench_session_remove.py's resident matrix: 1 000 000 x 100 000, about 1e8 nonzeros (uniform triplets, synth), k = 50, fp32.  Three
cases, each ONE call on the matrix the session started with (put back before every run, outside the clock):

    leave10         holdout(n_out=10) over all users
    frac20          holdout(frac=0.2) over all users
    leave10_4096    holdout(n_out=10, users=4096 of them)

Figures (each: a device-synchronised host clock around whole calls in one process, every route warmed up once, the median and the range of
`repeats` runs):

    call       (a) the call on the resident session: the held-out CSR comes back, the session holds the training matrix
    rebuild    (b) matrix(1) downloaded, the same Philox keys and the same selection in vectorised numpy, close, Session.from_coo(train),
               set_factors

Asserts that both routes hold identical training matrices in both orientations and return identical held-out matrices.  No ratio is asserted.
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

KINDS = ("leave10", "frac20", "leave10_4096")
USERS, SEED, MASK = 4096, 0x9E3779B97F4A7C15, np.uint64(0xFFFFFFFF)


def once(fn):
    """ms of one call of fn between device synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def figure(ms_list):
    return dict(ms=float(np.median(ms_list)), ms_min=float(min(ms_list)), ms_max=float(max(ms_list)), repeats=len(ms_list))


def philox_keys(items, users, seed):
    """section 2f's key of every (user, item) pair: Philox4x32-10 at counter (item, 1, user lo, user hi), vectorised"""
    s = np.uint64(32)
    c0, c1, c2, c3 = items.astype(np.uint64), np.ones(len(items), np.uint64), users.astype(np.uint64) & MASK, users.astype(np.uint64) >> s
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & MASK, (p0 >> s) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return (c0 << s) | c1


def held_out(ptr, ind, dimA, n_out, thresh, min_keep, users):
    """a flag per stored cell: section 2f's rule for the listed users (None: all), in numpy"""
    length = np.diff(ptr)
    rows = np.repeat(np.arange(dimA, dtype=np.int64), length)
    pick = np.ones(len(ind), bool) if users is None else np.isin(rows, users)
    at = np.flatnonzero(pick)
    r, j = rows[at], ind[at]
    keys = philox_keys(j, r, SEED)
    below = np.bincount(r, weights=(keys >> np.uint64(32)) < np.uint64(thresh) if thresh < 2 ** 32 else None, minlength=dimA).astype(np.int64)
    h = np.minimum(np.minimum(n_out, below), np.maximum(length - min_keep, 0))
    order = np.lexsort((j, keys, r))
    first = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=dimA))])[:-1]
    out = np.zeros(len(ind), bool)
    out[at[order]] = np.arange(len(at)) - first[r[order]] < h[r[order]]
    return out, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_holdout", "bench.json"))
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
    holder = {"s": api.Session.from_coo(trip, k, True)}
    del trip
    holder["s"].set_factors(A, B)
    val0, ind0, ptr0 = holder["s"].matrix(1)
    rows0 = np.repeat(np.arange(dimA, dtype=np.int64), np.diff(ptr0.astype(np.int64)))
    start = synth.Triplets(rows0, ind0.astype(np.int64), val0, (dimA, dimB))
    nnz0, longest = len(val0), int(np.diff(ptr0.astype(np.int64)).max())
    del rows0
    print(f"resident matrix: {nnz0} cells, longest user row {longest}", flush=True)

    def restore():
        holder["s"].close()
        holder["s"] = api.Session.from_coo(start, k, True)
        holder["s"].set_factors(A, B)

    some = np.sort(rng.permutation(dimA)[:USERS])
    cases = {"leave10": dict(n_out=10), "frac20": dict(frac=0.2), "leave10_4096": dict(n_out=10, users=some)}
    if args.calls_only:
        for kind in KINDS:
            T = holder["s"].holdout(seed=SEED, **cases[kind])
            print(f"{kind}: {T.nnz} cells held out, nnz {int(holder['s'].nnz(1))}", flush=True)
            restore()
        holder["s"].close()
        return
    out = {"workload": dict(dimA=dimA, dimB=dimB, k=k, nnz=nnz0, longest_user_row=longest, precision="fp32"),
           "method": "host clock around whole calls between device synchronisations, one process; routes warmed up; median of repeats; "
                     "the session is put back to the starting matrix before every run, outside the clock",
           "device": torch.cuda.get_device_name(0)}
    for kind in KINDS:
        kw = cases[kind]
        users = kw.get("users")
        n_out = kw.get("n_out", 2 ** 62)
        thresh = 2 ** 32 if "frac" not in kw else min(int(kw["frac"] * 2 ** 32), 2 ** 32)
        test = {}

        def call():
            test["call"] = holder["s"].holdout(seed=SEED, **kw)

        def rebuild():
            val, ind, ptr = holder["s"].matrix(1)
            ptr, ind = ptr.astype(np.int64), ind.astype(np.int64)
            flag, rows = held_out(ptr, ind, dimA, n_out, thresh, 1, users)
            T = sp.csr_matrix((val[flag], (rows[flag], ind[flag])), shape=(dimA, dimB))
            test["rebuild"] = T if users is None else T[users]
            keep = ~flag
            train = synth.Triplets(rows[keep], ind[keep], val[keep], (dimA, dimB))
            holder["s"].close()
            holder["s"] = api.Session.from_coo(train, k, True)
            holder["s"].set_factors(A, B)

        e = out[kind] = {}
        held = {}
        for route, fn in (("call", call), ("rebuild", rebuild)):
            ms = []
            for rep in range(args.repeats + 1):
                restore()
                ms.append(once(fn))
            e[route] = figure(ms[1:])
            held[route] = [holder["s"].matrix(w) for w in (1, 0)]
            print(f"{kind}: {route} {e[route]['ms']:.3f} ms [{e[route]['ms_min']:.3f}, {e[route]['ms_max']:.3f}]", flush=True)
        e["cells_held_out"], e["nnz_after"] = int(test["call"].nnz), len(held["call"][0][0])
        for a, b in zip(held["call"], held["rebuild"]):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), (kind, "the two routes hold different training matrices")
        a, b = test["call"], test["rebuild"].tocsr()
        b.sort_indices()
        assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) \
            and np.array_equal(a.data, b.data), (kind, "the two routes return different held-out matrices")
        assert e["nnz_after"] == nnz0 - e["cells_held_out"]
        del held, test
        e["rebuild_over_call"] = e["rebuild"]["ms"] / e["call"]["ms"]
        print(f"{kind}: {e['cells_held_out']} cells held out, ratio {e['rebuild_over_call']:.1f}", flush=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    holder["s"].close()


if __name__ == "__main__":
    main()
