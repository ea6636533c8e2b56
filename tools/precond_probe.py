"""Shift-preconditioner probe: cfg 3 (N = 50 000, 16 Gauss nodes, M0 = 64, residual target 1e-12) under
precond="shift" with precond_shifts 1, 2 and 4 against three baselines on the same build: plain solver="gmres", bench.py's cocg
settings, and solver="sparse_direct".  The variants run in ALTERNATING order (one solve of each per round, the order reversed
every other round) and the figure is the median over the rounds.  One JSON line per variant:

  ms per solve (median, min, max), loops, lock-steps per loop (the slowest node's), substitution sweeps and the device time of
  one (profiler class mf_solve / wband_solve / band_solve of the untimed first round, over the sweeps that round counted: ms
  per batched M^-1 of 16 x 64 columns; steps queued behind the last live column launch one too), the pivot factors' bytes,
  the device memory held after the solve, and for k_precond_op ms per launch and its algorithmic bytes per second as a fraction
  of the 4.8 TB/s copy ceiling bench.py quotes: for the cycle-start launches (class precond_op_start: every node is live, four
  N x 64 complex128 panels per node -- u, T, b in, r out -- and B's values once), and as an upper bound for the step launches
  (class precond_op: three panels per node, but nodes that left are skipped and the profiler does not say how many had).

  python tools/precond_probe.py [--rounds 5] [--variants shift1,shift2,shift4,gmres,cocg,direct] [--out profiles/precond_probe.txt]

The plain GMRES baseline is the only speed comparison the mode claims; its rounds are capped by --gmres-rounds (it is slow)."""
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

COPY_CEILING = 4.8e12
SUBST_CLASSES = ("mf_solve", "wband_solve", "band_solve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gmres-rounds", type=int, default=1)
    ap.add_argument("--variants", default="shift1,shift2,shift4,gmres,cocg,direct")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precond_probe.txt"))
    ap.add_argument("--grid", default="50,40,25")
    args = ap.parse_args()
    import torch
    import feast_oracle as fo
    import feastkit_jl_amd as fk

    nx, ny, nz = (int(v) for v in args.grid.split(","))
    A, B, lam = fo.cfg3_problem(nx, ny, nz)
    N = A.shape[0]
    inside = lam[(lam >= 0.0) & (lam <= 0.1775)]
    eng = fk.HipEngine(0)
    eng.set_problem(A, B)
    Q0 = eng.upload(fk.seeded_subspace(N, 64))

    def solve(name):
        fpm = fk.feastinit()
        fpm[2], fpm[4] = 16, 40
        common = dict(preloaded=True, Q0=Q0, real_projection=True)
        if name.startswith("shift"):
            return fk.feast_hip_hermitian(eng, A, B, 0.0, 0.1775, 64, fpm, solver="gmres", warm_start=False, precond="shift",
                                          precond_shifts=int(name[5:]), **common)
        if name == "gmres":
            return fk.feast_hip_hermitian(eng, A, B, 0.0, 0.1775, 64, fpm, solver="gmres", warm_start=False, **common)
        if name == "direct":
            return fk.feast_hip_hermitian(eng, A, B, 0.0, 0.1775, 64, fpm, solver="banded", **common)
        fpm[16], fpm[18] = 0, 4000                                   # bench.py's cocg settings
        return fk.feast_hip_hermitian(eng, A, B, 0.0, 0.1775, 64, fpm, solver="cocg", warm_start=True, inner_rtol=3e-2,
                                      solver_maxiter=50, node_assignment="balanced", column_groups="auto", **common)

    names = args.variants.split(",")
    rec = {n: {"ms": [], "res": None, "prof": {}, "held": 0} for n in names}
    for rnd in range(args.rounds + 1):                                # round 0 warms every variant up and is not timed
        order = names if rnd % 2 == 0 else names[::-1]
        for n in order:
            if n == "gmres" and rnd > args.gmres_rounds:
                continue
            if rnd == 0:                                              # the in-library profiler runs in the untimed round only
                eng.profile_reset()
                eng.profile_enable(True)
                eng.profile_set_period(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = solve(n)
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            free_b, total_b = torch.cuda.mem_get_info()
            if rnd == 0:
                eng.profile_enable(False)
                rec[n]["prof"] = {c: eng.profile_get(c) for c in SUBST_CLASSES + ("precond_op", "precond_op_start")}      # (total ms, launches)
                rec[n]["sweeps0"] = sum(e["substitution_sweeps"] for e in (r.stats.get("precond") or []))
            else:
                rec[n]["ms"].append(dt)
            rec[n]["res"] = r
            rec[n]["held"] = int(total_b - free_b)
            eng.free_factors()                                        # as api.feast does when the call returns
    lines = []
    for n in names:
        r, ms = rec[n]["res"], rec[n]["ms"]
        log = (r.stats.get("precond") or []) if isinstance(r.stats, dict) else []
        sub_ms, sub_n = max((rec[n]["prof"][c] for c in SUBST_CLASSES), key=lambda v: v[1])
        op_ms, op_n = rec[n]["prof"]["precond_op"]
        st_ms, st_n = rec[n]["prof"]["precond_op_start"]
        nnzB = B.nnz
        start_bytes = 16 * (4 * N * 64 * 16) + 16 * (8 * nnzB + 4 * nnzB)
        op_bytes = 16 * (3 * N * 64 * 16) + 16 * (8 * nnzB + 4 * nnzB)     # every node active: an upper bound on the traffic
        lines.append(json.dumps({
            "variant": n, "ok": bool(r.info == 0 and r.M == len(inside) and np.abs(np.sort(r.lambda_) - inside).max() <= 1e-9),
            "info": int(r.info), "M": int(r.M), "epsout": float(r.epsout),
            "ms_per_solve_median": round(float(np.median(ms)), 1) if ms else None, "ms_min": round(min(ms), 1) if ms else None,
            "ms_max": round(max(ms), 1) if ms else None, "timed_rounds": len(ms), "loops": int(r.loop) + 1,
            "lock_steps_per_loop": [max(e["lock_steps"]) for e in log] or [max(v) if v else 0 for v in r.stats.get("node_iterations", [])],
            "substitution_sweeps_per_loop": [e["substitution_sweeps"] for e in log],
            "substitution_ms_total": round(float(sub_ms), 2) if sub_n else None, "substitution_launches": int(sub_n),
            "substitution_ms_per_sweep": round(float(sub_ms) / rec[n]["sweeps0"], 3) if sub_n and rec[n].get("sweeps0") else None,
            "factorizations": int(r.stats.get("factorizations", 0)), "factor_bytes": log[0]["factor_bytes"] if log else None,
            "device_bytes_held_after_solve": rec[n]["held"],
            "precond_op_start_ms_each": round(float(st_ms) / st_n, 4) if st_n else None, "precond_op_start_launches": int(st_n),
            "precond_op_start_frac_of_copy_ceiling": round(start_bytes / (st_ms / st_n * 1e-3) / COPY_CEILING, 3) if st_n and st_ms > 0 else None,
            "precond_op_ms_each": round(float(op_ms) / op_n, 4) if op_n else None, "precond_op_launches": int(op_n),
            "precond_op_frac_of_copy_ceiling_upper_bound": round(op_bytes / (op_ms / op_n * 1e-3) / COPY_CEILING, 3) if op_n and op_ms > 0 else None}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/precond_probe.py --rounds %d --gmres-rounds %d --grid %s (N = %d, 16 nodes, M0 = 64, fpm[3] = 12)\n" %
                (args.rounds, args.gmres_rounds, args.grid, N))
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
