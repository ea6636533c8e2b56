#!/usr/bin/env python3
"""Wall time of the stochastic eigenvalue-count estimate (fpm[14] = 2) and of M0 = "auto" on cfg 3 (N = 50 000 3-D
Laplacian pencil, interval (0, 0.1775) holding 44 eigenvalues).  Stand-alone: bench.py does not call it.

  python tools/estimate_timing.py [--reps 3]

Prints one JSON line per measurement:
  estimate   64 samples on the estimate's 3-node contour, through the sparse direct solver (the estimate's default:
             multifrontal LU, factors released after the call) and through COCG from a zero start at inner tolerance
             1e-8; first call on a fresh engine (ingest + plan) and the median of the repeats
  auto       feast(A, B, (0, 0.1775), M0="auto", fpm[2] = 16) against the hand-set M0 = 64 call with the same parameters
             (the reference's default call shape: everything else at its default), medians of the repeats
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import feastkit_jl_amd as fk                                    # noqa: E402
from feastkit_jl_amd import workloads                           # noqa: E402

EMIN, EMAX = 0.0, 0.1775


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    A, B, lam = workloads.laplacian_3d_pencil()
    count = int(((lam >= EMIN) & (lam <= EMAX)).sum())

    def est_fpm():
        fpm = fk.feastinit()
        fpm[14] = 2
        return fpm

    for solver in ("direct", "cocg"):
        eng = fk.HipEngine(0)
        r, first = timed(lambda: fk.feast(A, B, (EMIN, EMAX), M0=64, fpm=est_fpm(), engine=eng, solver=solver))
        reps = []
        for _ in range(args.reps):
            r, t = timed(lambda: fk.feast(A, B, (EMIN, EMAX), M0=64, fpm=est_fpm(), engine=eng, solver=solver))
            reps.append(t)
        e = r.stats["estimate"]
        print(json.dumps({"what": "estimate", "solver_asked": solver, "solver": e["solver"], "nodes": e["nodes"],
                          "samples": len(e["samples"]), "mean": round(e["mean"], 3), "stderr": round(e["stderr"], 3),
                          "true_count": count, "ms_first_call": round(first * 1e3, 1),
                          "ms_median": round(float(np.median(reps)) * 1e3, 1),
                          "ms_in_estimate": round(e["seconds"] * 1e3, 1), "info": r.info}), flush=True)
        eng.close()

    eng = fk.HipEngine(0)
    rows = {}
    for tag, M0 in (("M0=64", 64), ("M0=auto", "auto")):
        times = []
        for _ in range(args.reps + 1):                         # the first call pays ingest and plan: not in the median
            fpm = fk.feastinit()
            fpm[2] = 16
            r, t = timed(lambda: fk.feast(A, B, (EMIN, EMAX), M0=M0, fpm=fpm, engine=eng))
            times.append(t)
        err = float(np.abs(np.sort(r.lambda_) - lam[:count]).max()) if r.M == count else None
        rows[tag] = {"ms_median": round(float(np.median(times[1:])) * 1e3, 1), "ms_first_call": round(times[0] * 1e3, 1),
                     "info": r.info, "M": r.M, "loops": r.loop, "max_eig_error": err,
                     "M0": r.stats.get("M0_auto", 64)}
        if M0 == "auto":
            e = r.stats["estimate"]
            rows[tag]["estimate"] = {"mean": round(e["mean"], 3), "stderr": round(e["stderr"], 3), "solver": e["solver"],
                                     "ms": round(e["seconds"] * 1e3, 1)}
    print(json.dumps({"what": "auto", "true_count": count, **rows}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
