#!/usr/bin/env python
"""feast_polynomial against feast_general on the explicit companion pencil: ms per solve as the median of five alternating
runs in one process, loops, M, the device time per profile class of one further solve of each, and the achieved bandwidth of
the poly_form kernel against the measured copy ceiling bench.py quotes.

Workload: a monic quadratic P(lambda) = (lambda - X_1)(lambda - X_2) at N = 4096 with a known spectrum (the construction of
tests/polynomial_cases.py: k = 24 eigenvalues inside the unit circle about 0.3 + 0.2i, the rest at 2.5 .. 4.5 radii), M0 = 24
(48 columns), 24 nodes, residual="reference" -- for a monic polynomial the measure of feast_general on the companion, so both
calls run the same loop from the same start block.  Both calls factor in every solve (keep_factors off).

    python tools/polynomial_probe.py                                     # both methods
    python tools/polynomial_probe.py --companion-only --package-root P   # the companion call on another checkout (the parent
                                                                         # commit: it has no feast_polynomial)

--workload sparse: the sparse path (solver="sparse_direct") on the cfg 3 grid.  (A, B, mu) = workloads.laplacian_3d_pencil(50,
40, 25), A_0 = A, A_1 = alpha B + beta A, A_2 = B (non-monic, N = 50 000): every pencil eigenvalue mu gives the two roots of
lambda^2 + (alpha + beta mu) lambda + mu = 0, so the spectrum is known.  The circle holds the roots of smallest positive
imaginary part up to the widest gap among the 8th .. 16th.  Comparator: feast_general on the explicit sparse 2N x 2N companion
through the sparse direct solver from the same start block (how the reference's feast_gcsrpev! does it); --companion-only
--package-root P runs that call alone on another checkout.  Also: k_spmm_fan's achieved GB/s on its algorithmic bytes in the
residual step, and that step's products as single-coefficient feasthip_matmul_dev calls on CSR handles holding A_k.

--method projected (either workload): feast_polynomial(..., method="projected") with --columns N-row columns (default 32 dense,
24 sparse) and a loop limit of 20, alternating with the linearised call as above (the comparator then is the linearised call,
not the companion pencil): ms per solve, loops, M, the per-loop history, rank and set-aside counts; then the achieved GB/s of
k_poly_resinv_acc (ne + 1 panels read, one written) and, sparse workload, of k_spmm_horner (nnz (4 + (d + 1) sizeof(VT)) plus
one panel written) on one 64-column panel, against the measured copy ceiling bench.py quotes.

--solver NAME [NAME ...] (--workload sparse --method projected; names of bicgstab, cocg, gmres): the projected method on Krylov
solves of P(z_e) x = r (no factors) at every --solver-tol, alternating with solver="sparse_direct" from the same start block in
one process: ms per solve, loops, Krylov iterations (total and the worst column per loop), capped nodes, and the device memory
each variant holds at the end of a solve on a handle of its own (hipMemGetInfo; the direct variant with its factors kept).
Then k_spmm_poly: device ms per launch on one node and on all nodes, 64 columns, against its algorithmic bytes nodes x (nnz (4 +
(d + 1) sizeof(VT)) + two panels), next to k_spmm on the pencil (A_0, A_d) of the same pattern (one node, 64 columns).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quadratic(N, k, seed=20260603):
    """Monic quadratic with k eigenvalues inside the circle (centre 0.3 + 0.2i, radius 1) -> (coeffs, centre, radius, inside)."""
    import numpy as np
    rng = np.random.default_rng([seed, N, k])
    c, r = 0.3 + 0.2j, 1.0
    inside = c + 0.8 * r * np.sqrt((np.arange(k) + 0.5) / k) * np.exp(1j * np.pi * (3.0 - np.sqrt(5.0)) * np.arange(k))
    Xs = []
    for i in range(2):
        ki = k // 2 + (k % 2 if i == 0 else 0)
        mu = np.empty(N, dtype=np.complex128)
        mu[:ki] = inside[i * (k // 2 + k % 2):][:ki]
        mu[ki:] = c + r * rng.uniform(2.5, 4.5, N - ki) * np.exp(2j * np.pi * rng.uniform(0, 1, N - ki))
        Z = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        Q, R = np.linalg.qr(Z)
        V = Q + (0.15 / np.sqrt(N)) * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
        Xs.append(np.linalg.solve(V.T, (V * mu).T).T)          # V diag(mu) V^-1
    A0 = Xs[0] @ Xs[1]
    A1 = -(Xs[0] + Xs[1])
    return [np.asfortranarray(A0), np.asfortranarray(A1), np.asfortranarray(np.eye(N, dtype=np.complex128))], c, r, inside


def companion(coeffs):
    import numpy as np
    N = coeffs[0].shape[0]
    A = np.zeros((2 * N, 2 * N), dtype=np.complex128, order="F")
    A[:N, N:] = np.eye(N)
    A[N:, :N] = -coeffs[0]
    A[N:, N:] = -coeffs[1]
    B = np.eye(2 * N, dtype=np.complex128)
    B[N:, N:] = coeffs[2]
    return A, np.asfortranarray(B)


CLASSES = ("poly_form", "poly_rhs", "poly_expand", "poly_residual", "poly_horner", "poly_resinv", "ortho", "lu_form", "lu_panel", "lu_laswp", "lu_trsm", "lu_gemm_in", "lu_gemm",
           "lu_invert", "lu_solve", "dense_op", "gram", "ritz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--M0", type=int, default=24)
    ap.add_argument("--nodes", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--maxloop", type=int, default=4)
    ap.add_argument("--companion-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT, help="checkout to import feastkit_jl_amd from")
    ap.add_argument("--workload", choices=("dense", "sparse"), default="dense")
    ap.add_argument("--grid", type=int, nargs=3, default=(50, 40, 25), help="sparse workload: nx ny nz")
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--beta", type=float, default=0.05)
    ap.add_argument("--method", choices=("linearised", "projected"), default="linearised")
    ap.add_argument("--columns", type=int, default=None, help="--method projected: N-row columns (default 32 dense, 24 sparse)")
    ap.add_argument("--solver", nargs="+", default=None, choices=("bicgstab", "cocg", "gmres"),
                    help="sparse workload, projected method: Krylov solvers on P(z) to set beside solver=sparse_direct")
    ap.add_argument("--solver-tol", type=float, nargs="+", default=(1e-4, 1e-2))
    ap.add_argument("--solver-maxiter", type=int, default=2000)
    ap.add_argument("--set-aside", type=float, nargs=2, default=None, metavar=("ABS", "FACTOR"),
                    help="experiment: run the projected method with these set-aside thresholds instead of POLY_SET_ASIDE")
    a = ap.parse_args()
    sys.path[:0] = [a.package_root]
    if a.set_aside is not None:
        import feastkit_jl_amd.hip_backend as hb
        hb.POLY_SET_ASIDE = (float(a.set_aside[0]), float(a.set_aside[1]))
    if a.solver:
        if a.workload != "sparse" or a.method != "projected":
            ap.error("--solver needs --workload sparse --method projected")
        return main_krylov(a)
    if a.workload == "sparse":
        return main_sparse(a)
    import numpy as np
    import feastkit_jl_amd as fk

    coeffs, center, radius, inside = quadratic(a.N, a.k)
    d, N = 2, a.N
    Alin, Blin = companion(coeffs)
    Q0 = fk.seeded_subspace(d * N, a.M0 * d)
    eng = fk.HipEngine(0)

    def fpm():
        f = fk.feastinit()
        f[8], f[4], f[3] = a.nodes, a.maxloop, 10
        return f

    def run(name):
        eng.synchronize()
        t0 = time.perf_counter()
        if name == "projected":
            f = fpm()
            f[4] = 20
            r = fk.feast_polynomial(coeffs, center, radius, M0=columns, fpm=f, engine=eng, method="projected")
        elif name == "polynomial":
            r = fk.feast_polynomial(coeffs, center, radius, M0=a.M0, fpm=fpm(), engine=eng, Q0=Q0, residual="reference")
        else:
            r = fk.feast_general(Alin, Blin, center, radius, M0=a.M0 * d, fpm=fpm(), engine=eng, Q0=Q0)
        eng.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    columns = a.columns or 32
    names = ("companion",) if a.companion_only else (("projected", "polynomial") if a.method == "projected" else ("polynomial", "companion"))
    for name in names:
        run(name)                                   # warm-up: kernels loaded, workspaces and factor slots made
    ms = {n: [] for n in names}
    last = {}
    for _ in range(a.runs):
        for name in names:
            last[name], t = run(name)
            ms[name].append(t)
    for name in names:
        r = last[name]
        lam_err = None
        if r.M == len(inside):
            left = list(inside)
            lam_err = 0.0
            for l in r.lambda_:
                j = int(np.argmin([abs(l - e) for e in left]))
                lam_err = max(lam_err, abs(l - left.pop(j)))
        row = {"method": name, "N": N, "degree": d, "M0": a.M0, "columns": a.M0 * d, "nodes": a.nodes, "ms_median": float(np.median(ms[name])),
               "ms_all": ms[name], "loops": r.loop, "M": r.M, "expected_M": len(inside), "info": r.info, "epsout": r.epsout,
               "factorizations": r.stats.get("factorizations"), "eigenvalue_error": lam_err,
               "factor_bytes": a.nodes * 16 * (N if name == "polynomial" else d * N) ** 2}
        if name in ("polynomial", "projected") and len(r.stats["polynomial"]["backward_error"]):
            row["backward_error_max"] = float(np.max(r.stats["polynomial"]["backward_error"]))
        if name == "projected":
            row.update(projected_fields(r, columns))
            row["factor_bytes"] = a.nodes * 16 * N ** 2
        print(json.dumps(row), flush=True)
    # device time per profile class: one further solve of each with every launch timed
    for name in names:
        eng.profile_enable(True)
        eng.profile_set_period(1)
        eng.profile_reset()
        _, t = run(name)
        prof = {}
        for cls in CLASSES:
            total, n = eng.profile_get(cls)
            if n:
                prof[cls] = {"ms": round(total, 3), "launches": n}
        eng.profile_enable(False)
        row = {"method": name, "profiled_solve_ms": t, "classes": prof}
        if "poly_form" in prof:
            # algorithmic traffic of one launch: d + 1 coefficient matrices read, one matrix per node written
            traffic = 16.0 * N * N * (d + 1 + a.nodes)
            gbs = traffic / (prof["poly_form"]["ms"] / prof["poly_form"]["launches"] * 1e-3) / 1e9
            row["poly_form"] = {"bytes_per_launch": traffic, "GB_per_s": round(gbs, 1), "fraction_of_copy_ceiling_4800": round(gbs / 4800.0, 4)}
        if "lu_form" in prof:
            traffic = 16.0 * N2(name, N, d) * (2 * a.nodes + a.nodes)       # A and B read per node, one matrix per node written
            gbs = traffic / (prof["lu_form"]["ms"] / prof["lu_form"]["launches"] * 1e-3) / 1e9
            row["lu_form"] = {"bytes_per_launch": traffic, "GB_per_s": round(gbs, 1), "fraction_of_copy_ceiling_4800": round(gbs / 4800.0, 4)}
        print(json.dumps(row), flush=True)
    if a.method == "projected" and not a.companion_only:
        projected_kernels(eng, fk, coeffs, center, radius, a.nodes, sparse=False)
    eng.close()


def projected_fields(r, columns):
    poly = r.stats["polynomial"]
    import feastkit_jl_amd.hip_backend as hb
    return {"set_aside_thresholds": list(hb.POLY_SET_ASIDE), "columns": columns, "eps_history": [float(e) for e in poly["eps_history"]], "rank": poly["rank"], "candidates": poly["candidates"],
            "set_aside": poly["set_aside"]}


def projected_kernels(eng, fk, coeffs, center, radius, nodes, sparse):
    """k_poly_resinv_acc and (sparse) k_spmm_horner on one 64-column panel: device ms per launch and GB/s on the algorithmic bytes"""
    import numpy as np
    d, N, m = len(coeffs) - 1, coeffs[0].shape[0], 64
    nnz = None
    if sparse:
        from feastkit_jl_amd.ingest import polynomial_union_csr
        union = polynomial_union_csr(coeffs)
        nnz = len(union[1])
        cplx = np.iscomplexobj(union[2][0])
        eng.set_polynomial_csr(*union)
    else:
        eng.set_polynomial(coeffs)
    eng.set_solver("direct", cache_factors=True, factor_precision=64)
    eng.set_real_projection(False)
    f = fk.feastinit()
    fk.feastdefault(f)
    f[8] = nodes
    Zne, Wne = fk.feast_gcontour(center, radius, f)
    eng.set_contour(Zne, Wne, 1.0)
    rng = np.random.default_rng(7)
    dX = eng.upload(np.asfortranarray(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))))
    sigma = center + 0.5 * radius * np.exp(2j * np.pi * (np.arange(m) + 0.25) / m)
    eng.poly_resinv_apply(dX, m, sigma)                          # warm-up: factors, workspaces
    eng.poly_eval_cols(dX, sigma, m)
    eng.profile_enable(True)
    eng.profile_set_period(1)
    reps = 10
    eng.profile_reset()
    for _ in range(reps):
        eng.poly_resinv_apply(dX, m, sigma)
    ms, n = eng.profile_get("poly_resinv")
    panel = 16.0 * N * m
    traffic = panel * (nodes + 2)
    row = {"what": "k_poly_resinv_acc", "N": N, "m": m, "nodes": nodes, "ms_per_launch": ms / n, "bytes_per_launch": traffic,
           "GB_per_s": traffic / (ms / n * 1e-3) / 1e9}
    row["fraction_of_copy_ceiling_4800"] = row["GB_per_s"] / 4800.0
    print(json.dumps(row), flush=True)
    if sparse:
        eng.profile_reset()
        for _ in range(reps):
            eng.poly_eval_cols(dX, sigma, m)
        ms, n = eng.profile_get("poly_horner")
        traffic = nnz * (4.0 + (d + 1) * (16 if cplx else 8)) + panel
        row = {"what": "k_spmm_horner", "N": N, "m": m, "nnz": nnz, "degree": d, "complex_values": bool(cplx), "ms_per_launch": ms / n,
               "bytes_per_launch": traffic, "GB_per_s": traffic / (ms / n * 1e-3) / 1e9, "gathered_bytes_per_launch": nnz * 16.0 * m}
        row["fraction_of_copy_ceiling_4800"] = row["GB_per_s"] / 4800.0
        print(json.dumps(row), flush=True)
    eng.profile_enable(False)
    eng.free_factors()


SPARSE_CLASSES = ("poly_spmm", "poly_mf_assemble", "poly_rhs", "poly_expand", "poly_residual", "poly_horner", "poly_resinv", "ortho", "mf_assemble", "mf_lu", "mf_solve", "spmm",
                  "gram", "ritz")


def sparse_quadratic(grid, alpha, beta):
    """-> (coeffs CSR, centre, radius, roots inside) of A + lambda (alpha B + beta A) + lambda^2 B on the Laplacian pencil"""
    import numpy as np
    import scipy.sparse as sp
    from feastkit_jl_amd import workloads
    A, B, mu = workloads.laplacian_3d_pencil(*grid)
    b = alpha + beta * mu
    root = np.sqrt((b * b - 4.0 * mu).astype(complex))
    lam = np.concatenate([(-b + root) / 2.0, (-b - root) / 2.0])
    up = lam[lam.imag > 1e-8]
    up = up[np.argsort(up.imag)]
    center = complex(np.mean(up[:8]))
    dist = np.sort(np.abs(lam - center))
    j = 7 + int(np.argmax(dist[8:17] - dist[7:16]))                  # the circle holds dist[0 .. j]
    radius = 0.5 * (dist[j] + dist[j + 1])
    inside = lam[np.abs(lam - center) <= radius]
    return [sp.csr_matrix(A), sp.csr_matrix(alpha * B + beta * A), sp.csr_matrix(B)], center, float(radius), inside


def sparse_companion(coeffs):
    import scipy.sparse as sp
    N = coeffs[0].shape[0]
    I = sp.identity(N, format="csr")
    A = sp.bmat([[None, I], [-coeffs[0], -coeffs[1]]], format="csr")
    B = sp.bmat([[I, None], [None, coeffs[2]]], format="csr")
    return A, B


def match_error(found, expected):
    import numpy as np
    if len(found) != len(expected):
        return None
    left, worst = list(expected), 0.0
    for l in found:
        j = int(np.argmin([abs(l - e) for e in left]))
        worst = max(worst, abs(l - left.pop(j)))
    return worst


def main_sparse(a):
    import numpy as np
    import feastkit_jl_amd as fk
    coeffs, center, radius, inside = sparse_quadratic(tuple(a.grid), a.alpha, a.beta)
    d, N = 2, coeffs[0].shape[0]
    M0 = len(inside)
    Alin, Blin = sparse_companion(coeffs)
    Q0 = fk.seeded_subspace(d * N, M0 * d)
    eng = fk.HipEngine(0)
    nodes = 16

    def fpm():
        f = fk.feastinit()
        f[8], f[4], f[3] = nodes, 20, 10
        return f

    def run(name):
        eng.synchronize()
        t0 = time.perf_counter()
        try:
            if name == "projected":
                r = fk.feast_polynomial(coeffs, center, radius, M0=columns, fpm=fpm(), engine=eng, solver="sparse_direct", method="projected")
            elif name == "polynomial":
                r = fk.feast_polynomial(coeffs, center, radius, M0=M0, fpm=fpm(), engine=eng, Q0=Q0, solver="sparse_direct")
            else:
                r = fk.feast_general(Alin, Blin, center, radius, M0=M0 * d, fpm=fpm(), engine=eng, Q0=Q0, solver="sparse_direct")
        except Exception as err:                    # does not fit, no plan: recorded, not tuned away
            return err, 1e3 * (time.perf_counter() - t0)
        eng.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    columns = a.columns or 24
    names = ("companion",) if a.companion_only else (("projected", "polynomial") if a.method == "projected" else ("polynomial", "companion"))
    for name in names:
        run(name)
    ms = {n: [] for n in names}
    last = {}
    for _ in range(a.runs):
        for name in names:
            last[name], t = run(name)
            ms[name].append(t)
    for name in names:
        r = last[name]
        row = {"workload": "sparse", "method": name, "grid": list(a.grid), "N": N, "order": N if name == "polynomial" else d * N, "M0": M0,
               "columns": M0 * d, "nodes": nodes, "ms_median": float(np.median(ms[name])), "ms_all": ms[name]}
        if isinstance(r, Exception):
            row["error"] = str(r)
        else:
            row.update(loops=r.loop, M=r.M, expected_M=len(inside), info=r.info, epsout=r.epsout, factorizations=r.stats.get("factorizations"),
                       eigenvalue_error=match_error(r.lambda_, inside), solver_substitution=r.stats.get("solver_substitution"))
            if name == "projected":
                row.update(projected_fields(r, columns))
            if name in ("polynomial", "projected") and len(r.stats["polynomial"]["backward_error"]):
                poly = r.stats["polynomial"]
                row.update(backward_error_max=float(np.max(poly["backward_error"])), plan=poly.get("plan"), fell_back=poly.get("fell_back"),
                           factor_bytes_per_node=poly.get("plan_factor_bytes"), flops_per_node=poly.get("plan_flops"), nnz=poly.get("plan_nnz"))
        print(json.dumps(row), flush=True)
    for name in names:
        eng.profile_enable(True)
        eng.profile_set_period(1)
        eng.profile_reset()
        _, t = run(name)
        prof = {}
        for cls in SPARSE_CLASSES:
            total, n = eng.profile_get(cls)
            if n:
                prof[cls] = {"ms": round(total, 3), "launches": n}
        eng.profile_enable(False)
        print(json.dumps({"workload": "sparse", "method": name, "profiled_solve_ms": t, "classes": prof}), flush=True)
    if a.method == "projected" and not a.companion_only:
        projected_kernels(eng, fk, coeffs, center, radius, nodes, sparse=True)
    elif not a.companion_only:
        fan_against_single_products(eng, fk, coeffs, M0 * d)
    eng.close()


def main_krylov(a):
    import numpy as np
    import torch
    import feastkit_jl_amd as fk
    from feastkit_jl_amd.ingest import polynomial_union_csr
    coeffs, center, radius, inside = sparse_quadratic(tuple(a.grid), a.alpha, a.beta)
    d, N = 2, coeffs[0].shape[0]
    columns = a.columns or 24
    nodes = 16
    Q0 = fk.seeded_subspace(N, columns)
    symmetric = all(abs(c - c.T).max() == 0 for c in coeffs)
    variants = [("sparse_direct", None)] + [(s, t) for s in a.solver for t in a.solver_tol if s != "cocg" or symmetric]
    if "cocg" in a.solver and not symmetric:
        print(json.dumps({"note": "cocg left out: a coefficient is not symmetric"}), flush=True)

    def fpm():
        f = fk.feastinit()
        f[8], f[4], f[3] = nodes, 20, 10
        return f

    def run(eng, v, **kw):
        eng.synchronize()
        t0 = time.perf_counter()
        extra = {} if v[1] is None else {"solver_tol": v[1], "solver_maxiter": a.solver_maxiter}
        try:
            r = fk.feast_polynomial(coeffs, center, radius, M0=columns, fpm=fpm(), engine=eng, Q0=Q0, solver=v[0], method="projected", **extra, **kw)
        except Exception as err:
            return err, 1e3 * (time.perf_counter() - t0)
        eng.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    # device memory per variant: a handle of its own, read at the end of one solve (which also warms the kernels up)
    mem = {}
    for v in variants:
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        e1 = fk.HipEngine(0)
        run(e1, v, keep_factors=True)
        free1, _ = torch.cuda.mem_get_info()
        mem[v] = int(free0 - free1)
        e1.free_factors()
        e1.close()
    eng = fk.HipEngine(0)
    for v in variants:
        run(eng, v)
    ms = {v: [] for v in variants}
    last = {}
    for _ in range(a.runs):
        for v in variants:
            last[v], t = run(eng, v)
            ms[v].append(t)
    for v in variants:
        r = last[v]
        row = {"workload": "sparse", "method": "projected", "solver": v[0], "solver_tol": v[1], "grid": list(a.grid), "N": N, "columns": columns,
               "nodes": nodes, "ms_median": float(np.median(ms[v])), "ms_all": ms[v], "device_bytes_held": mem[v]}
        if isinstance(r, Exception):
            row["error"] = str(r)
        else:
            poly = r.stats["polynomial"]
            row.update(loops=r.loop, M=r.M, expected_M=len(inside), info=r.info, epsout=r.epsout, factorizations=r.stats.get("factorizations"),
                       eigenvalue_error=match_error(r.lambda_, inside), eps_history=[float(e) for e in poly["eps_history"]], plan=poly.get("plan"),
                       krylov_iterations=r.stats.get("krylov_iterations"))
            if "krylov" in poly:
                row.update(worst_column_steps=[k["iterations"] for k in poly["krylov"]], capped_nodes=[k["capped_nodes"] for k in poly["krylov"]])
        print(json.dumps(row), flush=True)
    # device time per class of one further solve of each Krylov variant
    for v in variants[1:]:
        eng.profile_enable(True)
        eng.profile_set_period(1)
        eng.profile_reset()
        _, t = run(eng, v)
        prof = {}
        for cls in SPARSE_CLASSES + ("spmm_poly", "dot_finalize", "bicg_s", "bicg_xr", "bicg_p", "cocg_xr", "cocg_p", "gmres_ortho"):
            total, n = eng.profile_get(cls)
            if n:
                prof[cls] = {"ms": round(total, 3), "launches": n}
        eng.profile_enable(False)
        print(json.dumps({"workload": "sparse", "solver": v[0], "solver_tol": v[1], "profiled_solve_ms": t, "classes": prof}), flush=True)
    # k_spmm_poly on 64 columns, one node and all nodes, and k_spmm on the pencil of the same pattern
    union = polynomial_union_csr(coeffs)
    nnz, cplx, m, reps = len(union[1]), np.iscomplexobj(union[2][0]), 64, 20
    f = fpm()
    fk.feastdefault(f)
    Zne, Wne = fk.feast_gcontour(center, radius, f)
    rng = np.random.default_rng(7)
    panel = 16.0 * N * m
    eng.profile_enable(True)
    eng.profile_set_period(1)
    for ne in (1, nodes):
        eng.set_polynomial_csr(*union)
        eng.set_solver("direct")
        eng.set_contour(Zne[:ne], Wne[:ne], 1.0)
        dX = eng.upload(np.asfortranarray(rng.standard_normal((N, ne * m)) + 1j * rng.standard_normal((N, ne * m))))
        eng.poly_node_products(dX, m)
        eng.profile_reset()
        for _ in range(reps):
            eng.poly_node_products(dX, m)
        t, n = eng.profile_get("spmm_poly")
        traffic = ne * (nnz * (4.0 + (d + 1) * (16 if cplx else 8)) + 2 * panel)
        row = {"what": "k_spmm_poly", "N": N, "m": m, "nodes": ne, "nnz": nnz, "degree": d, "complex_values": bool(cplx), "ms_per_launch": t / n,
               "bytes_per_launch": traffic, "GB_per_s": traffic / (t / n * 1e-3) / 1e9, "gathered_bytes_per_launch": ne * nnz * 16.0 * m}
        row["fraction_of_copy_ceiling_4800"] = row["GB_per_s"] / 4800.0
        print(json.dumps(row), flush=True)
    eng.set_problem(coeffs[0], coeffs[d])
    dX = eng.upload(np.asfortranarray(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))))
    eng.matmul(0, dX, m)
    eng.profile_reset()
    for _ in range(reps):
        eng.matmul(0, dX, m)
    t, n = eng.profile_get("spmm")
    traffic = nnz * (4.0 + 2 * 8) + 2 * panel
    print(json.dumps({"what": "k_spmm (pencil of the same pattern, one node)", "N": N, "m": m, "ms_per_launch": t / n, "bytes_per_launch": traffic,
                      "GB_per_s": traffic / (t / n * 1e-3) / 1e9}), flush=True)
    eng.profile_enable(False)
    eng.close()


def fan_against_single_products(eng, fk, coeffs, m):
    """The residual step's products on one 64-column panel: d launches of k_spmm_fan (x_0 -> A_0 .. A_d, x_1 -> A_1, A_2) against
    the same 2 d + 2 products as single-coefficient feasthip_matmul_dev calls on CSR handles holding A_k."""
    import numpy as np
    from feastkit_jl_amd.ingest import polynomial_union_csr
    d, N = len(coeffs) - 1, coeffs[0].shape[0]
    m = min(m, 64)
    union = polynomial_union_csr(coeffs)
    nnz = len(union[1])
    eng.set_polynomial_csr(*union)
    eng.set_solver("direct")
    rng = np.random.default_rng(7)
    dX = eng.upload(np.asfortranarray(rng.standard_normal((d * N, m)) + 1j * rng.standard_normal((d * N, m))))
    V, lam = np.eye(m, dtype=complex), np.full(m, 0.1 + 0.5j)
    eng.poly_ritz_residual(dX, m, V, lam, m)                       # warm-up
    eng.profile_enable(True)
    eng.profile_set_period(1)
    reps = 10
    eng.profile_reset()
    for _ in range(reps):
        eng.poly_ritz_residual(dX, m, V, lam, m)
    fan_ms, fan_n = eng.profile_get("poly_spmm")
    ld = 16 if m <= 16 else (32 if m <= 32 else 64)
    panel = 16.0 * N * ld
    # per residual step: launch 1 (d + 1 outputs), launch 2 (2 outputs, one accumulating): matrix bytes + X read + Y written (+ read)
    bytes_step = (nnz * (4 + 8 * (d + 1)) + panel * (1 + d + 1)) + (nnz * (4 + 8 * 2) + panel * (1 + 2 + 1))
    row = {"workload": "sparse", "what": "residual-step products", "m": m, "ld": ld, "fan_ms_per_step": fan_ms / reps, "fan_launches_per_step": fan_n / reps,
           "fan_bytes_per_step": bytes_step, "fan_GB_per_s": bytes_step / (fan_ms / reps * 1e-3) / 1e9}
    row["fan_fraction_of_copy_ceiling_4800"] = row["fan_GB_per_s"] / 4800.0
    # the parent's way: one product per coefficient on CSR handles
    dx0 = eng.upload(np.ascontiguousarray(eng.download(dX, m)[:N]))
    single_ms, single_n = 0.0, 0
    for k, count in ((0, 2), (1, 2), (2, 2)):                       # A_0 x_0 twice (T, PK_0), A_1 x_1 and A_1 x_0, A_2 x_1 and A_2 x_0
        eng.set_problem(coeffs[k])
        eng.matmul(0, dx0, m)
        eng.profile_reset()
        for _ in range(reps * count):
            eng.matmul(0, dx0, m)
        t, n = eng.profile_get("spmm")
        single_ms += t / reps
        single_n += n / reps
    eng.profile_enable(False)
    row.update(single_ms_per_step=single_ms, single_launches_per_step=single_n, single_over_fan=single_ms / (fan_ms / reps))
    print(json.dumps(row), flush=True)


def N2(name, N, d):
    return float(N if name == "polynomial" else d * N) ** 2


if __name__ == "__main__":
    main()
