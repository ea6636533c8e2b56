"""Per-node solver probe: cfg 3 with bench.py's settings (16 Gauss nodes, M0 = 64, fpm[18] = 4000, COCG in sum mode, Ritz
warm start, inner_rtol 3e-2, cap 50) for direct_nodes in None, [15], [0, 15], "auto".  One JSON line per setting: ms per solve
(median and spread over the timed steps), loops, Krylov iterations, cocg_vec (k_fused_vec) launches per solve from the
in-library profiler, factorisations, the nodes chosen.  The cached factors are released after every solve, as api.feast does,
so every timed step pays its factorisations.

  python tools/node_solver_probe.py [--steps 5] [--warmup 1] [--settings none,15,0+15,auto]

`--settings none` runs without the keyword, so the same file measures a build that predates it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = {"none": None, "15": [15], "0+15": [0, 15], "auto": "auto"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--settings", default="none,15,0+15,auto")
    args = ap.parse_args()
    import torch
    import feast_oracle as fo
    import feastkit_jl_amd as fk

    A, B, lam = fo.cfg3_problem(50, 40, 25)
    inside = lam[(lam >= 0.0) & (lam <= 0.1775)]
    eng = fk.HipEngine(0)
    eng.set_problem(A, B)
    Q0 = eng.upload(fk.seeded_subspace(A.shape[0], 64))

    def step(spec):
        fpm = fk.feastinit()
        fpm[2], fpm[4], fpm[16], fpm[18] = 16, 40, 0, 4000
        kw = {} if spec is None else {"direct_nodes": spec}
        r = fk.feast_hip_hermitian(eng, A, B, 0.0, 0.1775, 64, fpm, solver="cocg", warm_start=True, inner_rtol=3e-2,
                                   solver_maxiter=50, preloaded=True, node_assignment="balanced", column_groups="auto",
                                   Q0=Q0, real_projection=True, **kw)
        eng.free_factors()
        return r

    for name in args.settings.split(","):
        spec = SETTINGS[name]
        for _ in range(args.warmup):
            step(spec)
        eng.profile_reset()
        eng.profile_enable(True)
        times, res = [], None
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = step(spec)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        eng.profile_enable(False)
        _, vec = eng.profile_get("cocg_vec")
        fin_ms, fin_n = eng.profile_get("node_finish")
        log = res.stats.get("direct_nodes") or []
        ok = bool(res.info == 0 and res.M == len(inside) and np.abs(np.sort(res.lambda_) - inside).max() <= 1e-10)
        print(json.dumps({
            "direct_nodes": name, "ok": ok, "ms_per_solve_median": round(float(np.median(times)), 2),
            "ms_min": round(min(times), 2), "ms_max": round(max(times), 2), "steps": args.steps, "loops": int(res.loop) + 1,
            "krylov_iterations": int(res.stats["krylov_iterations"]), "cocg_vec_launches_per_solve": int(vec) // max(args.steps, 1),
            "factorizations": int(res.stats["factorizations"]), "solve_seconds": round(float(res.stats["solve_seconds"]), 4),
            "node_finish_launches_per_solve": int(fin_n) // max(args.steps, 1),
            "nodes_per_loop": [e["nodes"] for e in log],
            "auto": [{k: e[k] for k in ("t_iter", "t_solve", "t_factor", "loops_left", "predicted_gain") if k in e} for e in log]
            if name == "auto" else None}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
