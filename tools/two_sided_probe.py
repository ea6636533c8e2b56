#!/usr/bin/env python
"""Two-sided against one-sided feast_general on cfg 5 (workloads.disc_spectrum_general(8192), circle centre 0 radius 2,
24 nodes, M0 = 48, fpm[4] = 20): ms per solve as the median of five alternating runs in one process, loops, M, and the
two-sided solve's split into forward sweep, adjoint sweep and Rayleigh-Ritz.  One JSON line per method on stdout.

    python tools/two_sided_probe.py                                            # timing
    rocprofv3 --kernel-trace --stats -- python tools/two_sided_probe.py --once two_sided    # device time per kernel: the
                                            # adjoint substitution kernels against their forward twins on the same factors
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np

import feastkit_jl_amd as fk


def solve(eng, A, two_sided, M0, nodes):
    fpm = fk.feastinit()
    fpm[8], fpm[4] = nodes, 20
    eng.synchronize()
    t0 = time.perf_counter()
    r = fk.feast_general(A, None, 0.0, 2.0, M0=M0, fpm=fpm, engine=eng, two_sided=two_sided)
    eng.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", default=None, choices=("one_sided", "two_sided"), help="one solve of this method (for a profiler run)")
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--M0", type=int, default=48)
    ap.add_argument("--nodes", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    A, delta = fk.workloads.disc_spectrum_general(a.N)
    A = np.asfortranarray(A)
    expected = int((np.abs(delta) <= 2.0).sum())
    eng = fk.HipEngine(0)
    if a.once:
        r, ms = solve(eng, A, a.once == "two_sided", a.M0, a.nodes)
        print(json.dumps({"method": a.once, "ms": ms, "loops": r.loop, "M": r.M, "expected_M": expected, "info": r.info}))
        return
    solve(eng, A, False, a.M0, a.nodes)              # warm-up: library load, buffers
    ms = {"one_sided": [], "two_sided": []}
    last = {}
    for _ in range(a.runs):
        for name in ("one_sided", "two_sided"):
            r, t = solve(eng, A, name == "two_sided", a.M0, a.nodes)
            ms[name].append(t)
            last[name] = r
    for name in ("one_sided", "two_sided"):
        r = last[name]
        row = {"method": name, "N": a.N, "M0": a.M0, "nodes": a.nodes, "ms_median": float(np.median(ms[name])), "ms_all": ms[name],
               "loops": r.loop, "M": r.M, "expected_M": expected, "info": r.info, "epsout": r.epsout,
               "factorizations": r.stats.get("factorizations")}
        if r.M:
            res = np.linalg.norm(A @ r.q - r.q * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
            row["max_right_residual_host"] = float(res.max())
        ts = r.stats.get("two_sided")
        if ts:
            row["seconds_last_solve"] = ts["seconds"]
            row["res_right"], row["res_left"] = ts["res_right"], ts["res_left"]
            row["adjoint_factorizations"] = ts["adjoint_factorizations"]
            row["biorthogonality"] = ts["biorthogonality"]
            row["min_overlap"] = float(np.min(ts["overlap"])) if len(ts["overlap"]) else None
        print(json.dumps(row))


if __name__ == "__main__":
    main()
