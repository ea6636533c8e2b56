"""Shifted COCG probe: the standard 3-D Laplacian at N = 50 000 (50 x 40 x 25, B = I) with bench.py's inner settings (16 Gauss
nodes, M0 = 64, fpm[18] = 4000, Ritz warm start, inner_rtol 3e-2, cap 50) and the interval that holds the bench's 44
eigenvalues, solved with solver="cocg" and solver="shifted_cocg" in the same process, interleaved step by step.

One JSON line per solver: ms per solve (median, min, max of the timed steps), loops, Krylov iterations summed over the
nodes, and for the shifted sweep the seed iterations (= SpMM node-passes).  Then one more, untimed, solve per solver with the
in-library profiler on: estimated device time and launches per kernel class, and for the vector kernel the algorithmic
bytes of the solve (from the per-(node, column) step counts of every loop), bytes per launch, and the fraction of the
4.8 TB/s read + write ceiling.

  python tools/shifted_probe.py [--steps 5] [--warmup 1] [--dims 50,40,25] [--solvers cocg,shifted_cocg]

Under `rocprofv3 --kernel-trace --stats -- python tools/shifted_probe.py --steps 1 --warmup 0` the same file gives the
per-kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CEILING = 4.8e12        # bytes / s, read + write
CLASSES = ("spmm", "dot_finalize", "cocg_vec", "shift_vec", "accumulate")


def vec_bytes(trace, N, ld, shifted):
    """Algorithmic bytes the vector kernel moves in one solve.  Per column step 16 B per row and pass.
    cocg (k_fused_vec): 5 passes per stepping (node, column) + the accumulator (2) per column that steps at any node.
    shifted (k_shift_vec): r read + write, q read and the accumulator read + write per column step of the seed recurrence
    (the longest node of the column), 2 passes per stepping (node, column)."""
    total = 0
    for t in trace:
        it = np.asarray(t["column_iterations"])                   # [node][column]
        longest = it.max(axis=0).sum()
        total += (3 + 2) * longest + 2 * it.sum() if shifted else 5 * it.sum() + 2 * longest
    return int(total) * 16 * N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", default="50,40,25")
    ap.add_argument("--solvers", default="cocg,shifted_cocg")
    args = ap.parse_args()
    import torch
    import feastkit_jl_amd as fk

    dims = [int(v) for v in args.dims.split(",")]
    A, lam = fk.workloads.laplacian_3d_standard(*dims)
    Emax = 0.1775 / (1.0 - 0.1 * 0.1775)                          # the bench's window in the eigenvalues of A itself
    inside = lam[(lam >= 0.0) & (lam <= Emax)]
    N = A.shape[0]
    eng = fk.HipEngine(0)
    eng.set_problem(A, None)
    Q0 = eng.upload(fk.seeded_subspace(N, 64))
    solvers = args.solvers.split(",")

    def step(solver, trace=None):
        fpm = fk.feastinit()
        fpm[2], fpm[4], fpm[16], fpm[18] = 16, 40, 0, 4000
        return fk.feast_hip_hermitian(eng, A, None, 0.0, Emax, 64, fpm, solver=solver, warm_start=True, inner_rtol=3e-2,
                                      solver_maxiter=50, preloaded=True, Q0=Q0, real_projection=True, trace=trace)

    for s in solvers:
        for _ in range(args.warmup):
            step(s)
    times = {s: [] for s in solvers}
    last = {}
    for _ in range(args.steps):                                   # interleaved: cocg, shifted, cocg, shifted, ...
        for s in solvers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[s] = step(s)
            torch.cuda.synchronize()
            times[s].append(1e3 * (time.perf_counter() - t0))
    for s in solvers:
        r, t = last[s], times[s]
        ok = bool(r.info == 0 and r.M == len(inside) and np.abs(np.sort(r.lambda_) - inside).max() <= 1e-10)
        sh = r.stats.get("shifted") or []
        print(json.dumps({
            "solver": s, "N": N, "ok": ok, "eigenpairs": int(r.M), "epsout": float(r.epsout),
            "ms_per_solve_median": round(float(np.median(t)), 2), "ms_min": round(min(t), 2), "ms_max": round(max(t), 2),
            "steps": args.steps, "loops": int(r.loop) + 1,
            "node_iterations_summed": int(sum(sum(v) for v in r.stats["node_iterations"])),
            "seed_iterations": int(sum(e["seed_iterations"] for e in sh)) if sh else None,
            "seed_node": sh[0]["seed_node"] if sh else None, "shifted_used": all(e["used"] for e in sh) if sh else None,
            "spmm_calls": int(r.stats["spmm_calls"])}), flush=True)
    for s in solvers:
        eng.profile_reset()
        eng.profile_enable(True)
        trace = []
        r = step(s, trace)
        torch.cuda.synchronize()
        eng.profile_enable(False)
        prof = {}
        for c in CLASSES:
            ms, n = eng.profile_get(c)
            if n:
                prof[c] = {"launches": int(n), "est_total_ms": round(float(ms), 2)}
        vec = "shift_vec" if s == "shifted_cocg" else "cocg_vec"
        out = {"solver": s, "profile": prof}
        if vec in prof and trace and trace[0].get("column_iterations") is not None:
            b = vec_bytes(trace, N, 64, s == "shifted_cocg")
            sec = prof[vec]["est_total_ms"] * 1e-3
            out["vector_kernel"] = {"class": vec, "alg_bytes_per_solve": b, "alg_bytes_per_launch": b // prof[vec]["launches"],
                                    "avg_launch_us": round(1e6 * sec / prof[vec]["launches"], 1),
                                    "alg_GBps": round(b / sec / 1e9, 1) if sec > 0 else None,
                                    "fraction_of_4p8TBps": round(b / sec / CEILING, 3) if sec > 0 else None}
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
