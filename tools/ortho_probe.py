"""Orthonormalisation probe: cfg 3 (3-D Laplacian 50 x 40 x 25, B = I + 0.1 A, 16 nodes, M0 = 64, the bench's interval with 44
eigenvalues) through the sparse direct solver on cached factors (solver="banded", keep_factors=True), where every refinement
loop orthonormalises a rank-deficient Q_proj.  ortho="mgs" and ortho="cholqr_rr" are timed alternately in one process, five
steps each after a warm-up that also factors the nodes.

One JSON line per method: wall ms per solve (median, min, max), loops, the Rayleigh-Ritz phases of the driver, and from the
in-library profiler (every launch timed, in an extra solve per step so that the wall times stay clean) the device ms per call
of the `ortho` class and of the `gram` class, plus what stats["ortho"] recorded.

  python tools/ortho_probe.py [--steps 5] [--warmup 1] [--dims 50,40,25]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METHODS = ("mgs", "cholqr_rr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", default="50,40,25")
    args = ap.parse_args()
    import torch
    import feastkit_jl_amd as fk

    dims = [int(v) for v in args.dims.split(",")]
    A, B, lam = fk.workloads.laplacian_3d_pencil(*dims)
    Emin, Emax, M0 = 0.0, 0.1775, 64
    inside = int(((lam >= Emin) & (lam <= Emax)).sum())
    eng = fk.HipEngine(0)

    def solve(method):
        fpm = fk.feastinit(); fpm[2] = 16
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fk.feast(A, B, (Emin, Emax), M0=M0, fpm=fpm, engine=eng, solver="banded", keep_factors=True, ortho=method)
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    wall = {m: [] for m in METHODS}
    dev = {m: {"ortho": [], "gram": []} for m in METHODS}
    last = {}
    for step in range(args.warmup + args.steps):
        for m in METHODS:
            r, ms = solve(m)
            assert r.info == 0 and r.M == inside, (m, r.info, r.M, inside)
            eng.profile_enable(True); eng.profile_set_period(1); eng.profile_reset()
            rp, _ = solve(m)
            per = {}
            for cls in ("ortho", "gram"):
                t, n = eng.profile_get(cls)
                per[cls] = t / (rp.loop + 1)                         # device ms of the class per orthonormalisation call
            eng.profile_enable(False)
            if step >= args.warmup:
                wall[m].append(ms)
                for cls in per:
                    dev[m][cls].append(per[cls])
            last[m] = r
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    for m in METHODS:
        r = last[m]
        ph = r.stats.get("phase_seconds", {})
        print(json.dumps({"ortho": m, "dims": dims, "M0": M0, "M": int(r.M), "loops": int(r.loop), "steps": args.steps,
                          "wall_ms_per_solve": stat(wall[m]),
                          "device_ms_per_call": {cls: stat(dev[m][cls]) for cls in dev[m]},
                          "phase_ms_last_solve": {k: round(1e3 * ph.get(k, 0.0), 2) for k in ("apply", "project", "ortho", "eig", "ritz")},
                          "stats_ortho": r.stats.get("ortho")}))
    d = float(np.abs(np.sort(last["mgs"].lambda_) - np.sort(last["cholqr_rr"].lambda_)).max())
    print(json.dumps({"max_eigenvalue_difference": d}))
    eng.free_factors()


if __name__ == "__main__":
    main()
