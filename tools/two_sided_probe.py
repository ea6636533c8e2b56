#!/usr/bin/env python
"""Two-sided against one-sided feast_general: ms per solve as the median of five alternating runs in one process, loops, M,
and the two-sided solve's split into forward sweep, adjoint sweep and Rayleigh-Ritz.  One JSON line per method on stdout.

  --workload dense  (default)  cfg 5: workloads.disc_spectrum_general(8192), circle centre 0 radius 2, 24 nodes, M0 = 48
  --workload sparse            the cfg 3 grid (50 x 40 x 25, N = 50 000) with a convection term in x (central differences,
                               coefficient 0.05: tridiag(-1.05, 2, -0.95) along x), B = I + 0.1 A, the circle over (0, 0.1775),
                               16 nodes, M0 = 64: sparse input under solver="direct", which the sparse direct solver takes with
                               its multifrontal plan.  Also printed: forward and adjoint contour_apply on the SAME cached
                               factors (median of five alternating sweeps), and the first adjoint product of the handle (the
                               lazy build of the conjugate-transposed CSR set) against the second.
  --workload sparse --plan band  the same in a child process with FH_MF_MAX_MULTIPLIER=0: the multifrontal LU rejects every
                               matrix, so every solve and both sweeps run on the blocked band LU (kl = ku = 951 after reverse
                               Cuthill-McKee); each solve then includes the rejected multifrontal factorisation.

    python tools/two_sided_probe.py [--workload sparse]                        # timing
    rocprofv3 --kernel-trace --stats -- python tools/two_sided_probe.py --once two_sided    # device time per kernel: the
                                            # adjoint substitution kernels against their forward twins on the same factors
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np

import feastkit_jl_amd as fk


def convection_pencil(nx=50, ny=40, nz=25, c=0.05, shift=0.1):
    """(A, B, lam): the 7-point Laplacian of cfg 3 with tridiag(-1 - c, 2, -1 + c) along x, B = I + shift A; the spectrum is
    real and known: mu = 2 - 2 sqrt(1 - c^2) cos(k pi / (nx + 1)) + the y and z terms, lam = mu / (1 + shift mu)."""
    import scipy.sparse as sp

    def t(n, cc=0.0):
        return sp.diags([(-1.0 - cc) * np.ones(n - 1), 2 * np.ones(n), (-1.0 + cc) * np.ones(n - 1)], [-1, 0, 1], format="csr")
    Ix, Iy, Iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = sp.csr_matrix(sp.kron(Iz, sp.kron(Iy, t(nx, c))) + sp.kron(Iz, sp.kron(t(ny), Ix)) + sp.kron(t(nz), sp.kron(Iy, Ix)))
    A.sort_indices()
    B = sp.csr_matrix(sp.identity(A.shape[0], format="csr") + shift * A)
    B.sort_indices()
    mx = 2 - 2 * np.sqrt(1 - c * c) * np.cos(np.arange(1, nx + 1) * np.pi / (nx + 1))
    my = 2 - 2 * np.cos(np.arange(1, ny + 1) * np.pi / (ny + 1))
    mz = 2 - 2 * np.cos(np.arange(1, nz + 1) * np.pi / (nz + 1))
    mu = np.sort((mx[:, None, None] + my[None, :, None] + mz[None, None, :]).ravel())
    return A, B, mu / (1 + shift * mu)


def solve(eng, A, B, center, radius, two_sided, M0, nodes):
    fpm = fk.feastinit()
    fpm[8], fpm[4] = nodes, 20
    eng.synchronize()
    t0 = time.perf_counter()
    r = fk.feast_general(A, B, center, radius, M0=M0, fpm=fpm, engine=eng, two_sided=two_sided)
    eng.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def sparse_sweeps(A, B, center, radius, M0, nodes, runs):
    """Engine-level figures on the sparse workload: the first adjoint product against the second, then forward and adjoint
    contour_apply alternating on the same cached multifrontal factors."""
    from feastkit_jl_amd.contour import feast_gcontour
    fpm = fk.feastinit()
    fpm[8] = nodes
    fk.feastdefault(fpm)
    Zne, Wne = feast_gcontour(complex(center), float(radius), fpm)
    eng = fk.HipEngine(0)
    try:
        eng.require_adjoint(True)
        eng.set_problem(A.astype(np.complex128), B.astype(np.complex128))
        eng.set_contour(Zne, Wne, 1.0)
        eng.set_real_projection(False)
        eng.set_node_range(0, len(Zne))
        eng.set_solver("banded")
        dQ = eng.upload(fk.seeded_subspace(A.shape[0], M0))
        eng.matmul(1, dQ, M0)                               # forward product: kernels loaded, buffers made
        eng.synchronize()
        first = []
        eng.set_adjoint(True)
        for _ in range(2):
            t0 = time.perf_counter()
            eng.matmul(1, dQ, M0)
            eng.synchronize()
            first.append(1e3 * (time.perf_counter() - t0))
        eng.set_adjoint(False)
        fwd, adj, nfact = [], [], []
        for k in range(runs + 1):                           # k = 0 factors (forward) and warms the adjoint kernels up
            for on in (False, True):
                eng.set_adjoint(on)
                eng.synchronize()
                t0 = time.perf_counter()
                _, status, st = eng.contour_apply(dQ, M0)
                eng.synchronize()
                ms = 1e3 * (time.perf_counter() - t0)
                nfact.append(int(st["factorizations"]))
                if k:
                    (adj if on else fwd).append(ms)
        eng.set_adjoint(False)
        plan = eng.band_plan()[3]                           # after the sweeps: the factors that ran (1 band, 2 multifrontal)
        print(json.dumps({"method": "sweeps_on_cached_factors", "direct_plan_blocked": plan, "nodes": len(Zne), "M0": M0,
                          "first_adjoint_product_ms": first[0], "second_adjoint_product_ms": first[1],
                          "forward_sweep_ms_median": float(np.median(fwd)), "adjoint_sweep_ms_median": float(np.median(adj)),
                          "adjoint_over_forward": float(np.median(adj) / np.median(fwd)), "forward_sweep_ms_all": fwd,
                          "adjoint_sweep_ms_all": adj, "factorizations_per_call": nfact, "worst_status": int(np.max(status))}))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", default=None, choices=("one_sided", "two_sided"), help="one solve of this method (for a profiler run)")
    ap.add_argument("--workload", default="dense", choices=("dense", "sparse"))
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--M0", type=int, default=None)
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--plan", default="library", choices=("library", "band"),
                    help="band (sparse workload): run in a child with FH_MF_MAX_MULTIPLIER=0, i.e. on the band LU's factors")
    a = ap.parse_args()
    if a.plan == "band":
        if a.workload != "sparse":
            ap.error("--plan band needs --workload sparse")
        if os.environ.get("FH_MF_MAX_MULTIPLIER") != "0":
            args = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
            sys.exit(subprocess.run(args, env=dict(os.environ, FH_MF_MAX_MULTIPLIER="0")).returncode)
    if a.workload == "sparse":
        A, B, lam = convection_pencil()
        center, radius = 0.08875, 0.08875
        expected = int((np.abs(lam - center) < radius).sum())
        M0, nodes = a.M0 or 64, a.nodes or 16
    else:
        A, delta = fk.workloads.disc_spectrum_general(a.N)
        A, B = np.asfortranarray(A), None
        center, radius = 0.0, 2.0
        expected = int((np.abs(delta) <= 2.0).sum())
        M0, nodes = a.M0 or 48, a.nodes or 24
    N = A.shape[0]
    eng = fk.HipEngine(0)
    if a.once:
        r, ms = solve(eng, A, B, center, radius, a.once == "two_sided", M0, nodes)
        print(json.dumps({"method": a.once, "workload": a.workload, "ms": ms, "loops": r.loop, "M": r.M, "expected_M": expected, "info": r.info}))
        return
    solve(eng, A, B, center, radius, False, M0, nodes)              # warm-up: library load, buffers
    ms = {"one_sided": [], "two_sided": []}
    last = {}
    for _ in range(a.runs):
        for name in ("one_sided", "two_sided"):
            r, t = solve(eng, A, B, center, radius, name == "two_sided", M0, nodes)
            ms[name].append(t)
            last[name] = r
    for name in ("one_sided", "two_sided"):
        r = last[name]
        row = {"method": name, "workload": a.workload, "N": N, "M0": M0, "nodes": nodes, "ms_median": float(np.median(ms[name])), "ms_all": ms[name],
               "loops": r.loop, "M": r.M, "expected_M": expected, "info": r.info, "epsout": r.epsout,
               "factorizations": r.stats.get("factorizations"), "solver_substitution": r.stats.get("solver_substitution")}
        if r.M:
            BX = r.q if B is None else B @ r.q
            res = np.linalg.norm(A @ r.q - BX * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
            row["max_right_residual_host"] = float(res.max())
        ts = r.stats.get("two_sided")
        if ts:
            row["seconds_last_solve"] = ts["seconds"]
            row["res_right"], row["res_left"] = ts["res_right"], ts["res_left"]
            row["adjoint_factorizations"] = ts["adjoint_factorizations"]
            row["biorthogonality"] = ts["biorthogonality"]
            row["min_overlap"] = float(np.min(ts["overlap"])) if len(ts["overlap"]) else None
            row["direct_plan"] = ts.get("direct_plan")
            row["fell_back"] = ts.get("fell_back")
        print(json.dumps(row), flush=True)
    eng.close()
    if a.workload == "sparse":
        sparse_sweeps(A, B, center, radius, M0, nodes, a.runs)


if __name__ == "__main__":
    main()
