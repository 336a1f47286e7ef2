#!/usr/bin/env python3
"""Time method "mm" (include/poismf_hip.h section 0) against PG on the headline matrix, in one process.

    python scripts/bench_mm.py [--out profiles/mm/bench.json] [--repeats 5] [--sweeps 10] [--race 20]

The workload of bench.py's headline: 10^6 x 10^5, 10^8 triplets (synth.uniform_triplets, seed 1), k = 50, fp32, maxupd 10, the factors
of harness.initialize_matrices.  PG runs with the settings that keep this matrix's factors alive (bench.py, PG_LIVE: l2 1e3, step 1e-9) and
is the parent commit's PG; "mm" runs with the same l2 and has no step.  fp64 and other k are not timed.

    pg_ms_per_sweep / mm_ms_per_sweep   a device-synchronised host clock around `--sweeps` sweeps (B half + A half) from the same start, after a
                                        warm-up of two; `--repeats` repeats with the two methods alternated inside each; median (min .. max)
    race                                after each of `--race` sweeps from the same start, per method: the training log-likelihood (Session.llk) and
                                        the objective both methods descend on, -llk over ALL cells + l2 (|A|^2 + |B|^2); and the first sweep at
                                        which each reaches the lower of the two final log-likelihoods / the higher of the two final objectives

No ratio is asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from poismf_amd import api, harness, synth

L2, STEP0, MAXUPD = 1e3, 1e-9, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mm", "bench.json"))
    ap.add_argument("--dimA", type=int, default=10 ** 6)
    ap.add_argument("--dimB", type=int, default=10 ** 5)
    ap.add_argument("--nnz", type=int, default=10 ** 8)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--race", type=int, default=20)
    args = ap.parse_args()
    torch.cuda.init()
    trip = synth.uniform_triplets(args.dimA, args.dimB, args.nnz, seed=1)
    sess = api.Session.from_coo(trip, args.k, True)
    del trip
    A0, B0 = harness.initialize_matrices(args.dimA, args.dimB, args.k, True, 1)
    params = {m: sess.make_params(m, L2, maxupd=MAXUPD, step_size=STEP0, limit_step=True, reuse_prev=True) for m in ("pg", "mm")}

    def objective():
        A, B = sess.get_factors()
        return -sess.llk(include_missing=True) + L2 * (float(np.square(A, dtype=np.float64).sum()) + float(np.square(B, dtype=np.float64).sum()))

    def sweeps(method, n, llk=False):
        """n sweeps from the common start; the time in ms per sweep, or (log-likelihood, objective) after each"""
        sess.set_factors(A0, B0)
        step, out = STEP0, []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step = sess.sweep(params[method], step)
            if llk:
                out.append((sess.llk(), objective()))
        torch.cuda.synchronize()
        return out if llk else (time.perf_counter() - t0) * 1e3 / n

    ms = {"pg": [], "mm": []}
    for m in ms:
        sweeps(m, 2)
    for _ in range(args.repeats):
        for m in ms:
            ms[m].append(sweeps(m, args.sweeps))
    race = {m: sweeps(m, args.race, llk=True) for m in ms}
    target = min(race["pg"][-1][0], race["mm"][-1][0])
    target_obj = max(race["pg"][-1][1], race["mm"][-1][1])
    out = {"workload": dict(dimA=args.dimA, dimB=args.dimB, k=args.k, nnz=int(sess.nnz(1)), dtype="fp32", maxupd=MAXUPD, l2=L2, pg_step0=STEP0),
           "method": "host clock around whole sweeps between device synchronisations; methods alternated; median (min .. max) of the repeats",
           "device": torch.cuda.get_device_name(0), "sweeps_per_figure": args.sweeps, "repeats": args.repeats}
    for m in ms:
        out[f"{m}_ms_per_sweep"] = dict(median=statistics.median(ms[m]), min=min(ms[m]), max=max(ms[m]))
    out["mm_over_pg"] = out["mm_ms_per_sweep"]["median"] / out["pg_ms_per_sweep"]["median"]
    out["race"] = {"target_llk": target, "target_objective": target_obj,
                   "llk_per_sweep": {m: [v[0] for v in race[m]] for m in ms}, "objective_per_sweep": {m: [v[1] for v in race[m]] for m in ms},
                   "sweeps_to_target_llk": {m: next(i + 1 for i, v in enumerate(race[m]) if v[0] >= target) for m in ms},
                   "sweeps_to_target_objective": {m: next(i + 1 for i, v in enumerate(race[m]) if v[1] <= target_obj) for m in ms}}
    sess.set_factors(A0, B0)
    out["race"]["llk_start"], out["race"]["objective_start"] = sess.llk(), objective()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    sess.close()


if __name__ == "__main__":
    main()
