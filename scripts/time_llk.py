#!/usr/bin/env python3
"""Time Session.llk (the Poisson log-likelihood, include/poismf_hip.h section 1e) against one PG(1) A half-sweep on the same session
(development aid).

    python scripts/time_llk.py [--repeats 10] [--nnz 100000000]

The C3 matrix (synth: uniform 1e6 x 1e5, 1e8 triplets), fp32, k = 50, one session.  Both gather one B row per nonzero, so they are
comparable.  After a warm-up the two are timed alternately, each by the wall clock between device-wide synchronisations (llk's own
8-byte copy back included).  Prints ms (median, min, max over the repeats) and llk's fraction of the byte roofline
nnz (k 4 + 4 + 4) + dimA k 4 bytes at 8 TB/s, then one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from poismf_amd import api, harness, synth

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    args = ap.parse_args()
    k, dimA, dimB = args.k, args.dimA, args.dimB
    torch.cuda.init()
    trip = synth.uniform_triplets(dimA, dimB, args.nnz, seed=1)
    sess = api.Session.from_coo(trip, k, True)
    del trip
    A, B = harness.initialize_matrices(dimA, dimB, k, True, 1)
    sess.set_factors(A, B)
    nnz = sess.nnz(1)
    l2, step = 1e3, 1e-9   # (bench.py's finite PG block: the factors stay positive, so every log is a real one)
    params = sess.make_params("pg", l2, step_size=step, maxupd=1)
    cnst = sess.cnst_div(l2, step)

    def t_llk():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = sess.llk()
        return (time.perf_counter() - t0) * 1e3, v

    def t_half():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.half_sweep(1, params, sess.real(step), cnst)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        t_llk()
        t_half()
    sess.set_factors(A, B)   # (the timed half-sweeps move A; the llk repeats are timed on whatever A is then)
    llk_ms, half_ms, vals = [], [], []
    for _ in range(args.repeats):
        ms, v = t_llk()
        llk_ms.append(ms)
        vals.append(v)
        half_ms.append(t_half())
    sess.close()
    nbytes = nnz * (k * 4 + 4 + 4) + dimA * k * 4
    med = float(np.median(llk_ms))
    res = {
        "what": "Session.llk vs one PG(1) A half-sweep, C3 matrix fp32 k=50, one session",
        "nnz": int(nnz), "dimA": dimA, "dimB": dimB, "k": k, "repeats": args.repeats,
        "llk_ms": {"median": med, "min": min(llk_ms), "max": max(llk_ms)},
        "pg1_A_half_ms": {"median": float(np.median(half_ms)), "min": min(half_ms), "max": max(half_ms)},
        "llk_bytes": int(nbytes),
        "llk_roofline_fraction": nbytes / (med * 1e-3) / HBM_BYTES_PER_S,
        "llk_roofline_fraction_best": nbytes / (min(llk_ms) * 1e-3) / HBM_BYTES_PER_S,
        "llk_first_value": vals[0],
    }
    print(f"Session.llk      {med:8.3f} ms median  [{min(llk_ms):.3f} .. {max(llk_ms):.3f}]  "
          f"{res['llk_roofline_fraction'] * 100:.1f} % of {nbytes / 1e9:.2f} GB at 8 TB/s")
    print(f"PG(1) A half     {res['pg1_A_half_ms']['median']:8.3f} ms median  [{min(half_ms):.3f} .. {max(half_ms):.3f}]")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
