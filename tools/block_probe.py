#!/usr/bin/env python
"""Block COCG against the per-column COCG sweep on the bench's flagship problem (cfg 3: laplacian_3d_pencil(50, 40, 25),
M0 = 64, 16 nodes, warm start, inner_rtol 3e-2, cap 50): ms per solve as the median of five alternating runs, per-node block
steps, breakdown nodes and loop counts.  One JSON line per solver on stdout.

    python tools/block_probe.py                      # timing
    rocprofv3 --kernel-trace --stats -- python tools/block_probe.py --once block_cocg     # device time of the new kernels
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import numpy as np

import feastkit_jl_amd as fk


def solve(A, B, interval, solver):
    fpm = fk.feastinit()
    fpm[2], fpm[16], fpm[18] = 16, 0, 4000
    t0 = time.perf_counter()
    r = fk.feast(A, B, interval, M0=64, fpm=fpm, solver=solver, warm_start=True, inner_rtol=3e-2, solver_maxiter=50)
    return r, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", default=None, help="one solve with this solver (for a profiler run)")
    ap.add_argument("--dims", default="50,40,25")
    a = ap.parse_args()
    dims = tuple(int(v) for v in a.dims.split(","))
    A, B, lam = fk.workloads.laplacian_3d_pencil(*dims)[:3]
    interval = (0.0, 0.1775)
    if a.once:
        r, ms = solve(A, B, interval, a.once)
        print(json.dumps({"solver": a.once, "ms": ms, "loops": r.loop, "M": r.M, "info": r.info}))
        return
    solve(A, B, interval, "cocg")                    # warm-up: library load, buffers
    ms = {"cocg": [], "block_cocg": []}
    last = {}
    for _ in range(5):
        for s in ("cocg", "block_cocg"):
            r, t = solve(A, B, interval, s)
            ms[s].append(t)
            last[s] = r
    for s in ("cocg", "block_cocg"):
        r = last[s]
        row = {"solver": s, "ms_median": float(np.median(ms[s])), "ms_all": ms[s], "loops": r.loop, "M": r.M, "info": r.info,
               "epsout": r.epsout, "node_iterations": r.stats.get("node_iterations")}
        if "block" in r.stats:
            row["block"] = r.stats["block"]
        print(json.dumps(row))


if __name__ == "__main__":
    main()
