"""Measurements for feast_nonlinear; needs the GPU.  One JSON line per measurement.

(a) the dense formation kernel of a term handle (profile class terms_form, k_form_terms) on N = 4096, 24 nodes, 3 terms, against
    poly_form (k_form_poly) on a quadratic of the same size in the same run -- the byte counts are identical: 3 matrices read,
    24 written -- and against a device-to-device copy of the same byte count timed in the same run.
(b) the N = 50 000 sparse quadratic of tools/polynomial_probe.py posed as terms, feast_nonlinear(solver="sparse_direct"), against
    feast_polynomial(method="projected", solver="sparse_direct") on the same engine, alternating, median of --runs; the host share
    of the nonlinear run (stats["nonlinear"]["reduced_seconds"]) and the device time per profile class of one further run of each.
(c) a delay problem on the same grid, A - lambda B + c e^{-tau lambda} B on the Laplacian pencil (A, B) of the workload: every
    pencil eigenvalue mu gives the roots mu + W_b(tau c e^{-tau mu}) / tau; loops, time and the eigenvalue error against them.

    python tools/nonlinear_probe.py [--runs 5] [--grid 50 40 25] [--skip a b c]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

CLASSES = ("terms_form", "poly_form", "terms_mf_assemble", "poly_mf_assemble", "mf_assemble", "terms_spmm", "poly_horner", "poly_spmm",
           "poly_resinv", "gram", "ritz", "lu_panel", "lu_gemm", "lu_gemm_in", "lu_trsm")


def classes(eng):
    out = {}
    for cls in CLASSES:
        total, n = eng.profile_get(cls)
        if n:
            out[cls] = {"ms": round(total, 3), "launches": n}
    return out


def profiled(eng, call):
    eng.profile_enable(True)
    eng.profile_set_period(1)
    eng.profile_reset()
    call()
    out = classes(eng)
    eng.profile_enable(False)
    return out


def form_kernels(eng, fk, np, N, nodes):
    import torch
    rng = np.random.default_rng(7)
    mats = [np.asfortranarray(rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) for _ in range(3)]
    mats[0] += 40.0 * np.eye(N)
    fpm = fk.feastinit()
    fpm[8] = nodes
    fk.feastdefault(fpm)
    Zne, Wne = fk.feast_gcontour(0.0 + 0j, 1.0, fpm)
    dX = eng.upload(rng.standard_normal((N, 16)) + 0j)
    traffic = 16.0 * N * N * (3 + nodes)
    row = {"measurement": "a", "N": N, "nodes": nodes, "terms": 3, "bytes_per_launch": traffic}
    for name in ("terms", "poly", "terms", "poly"):          # each twice, alternating; the second timing of each is kept
        if name == "terms":
            eng.set_terms(mats)
        else:
            eng.set_polynomial(mats)
        eng.set_solver("direct", cache_factors=True, factor_precision=64)
        eng.set_real_projection(False)
        eng.set_contour(Zne, Wne, 1.0)
        if name == "terms":
            eng.nep_set_node_values(np.stack([np.ones(nodes), Zne, np.exp(-Zne)], axis=1))
        call = (lambda: eng.nep_resinv_apply(dX, 16)) if name == "terms" else (lambda: eng.poly_resinv_apply(dX, 16))
        prof = profiled(eng, call)[name + "_form"]
        ms = prof["ms"] / prof["launches"]
        row[name + "_form"] = {"ms": round(ms, 4), "GB_per_s": round(traffic / (ms * 1e-3) / 1e9, 1)}
        eng.free_factors()
    eng.set_problem(np.eye(4))
    n = int(traffic // 32)                                   # a copy that reads and writes `traffic` bytes in all
    src = torch.empty(n, dtype=torch.complex128, device=eng.device)
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    best = None
    for _ in range(5):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        best = ev[0].elapsed_time(ev[1]) if best is None else min(best, ev[0].elapsed_time(ev[1]))
    row["copy"] = {"ms": round(best, 4), "GB_per_s": round(traffic / (best * 1e-3) / 1e9, 1)}
    for name in ("terms_form", "poly_form"):
        row[name]["fraction_of_copy"] = round(row[name]["GB_per_s"] / row["copy"]["GB_per_s"], 4)
    print(json.dumps(row), flush=True)


def sparse_runs(eng, fk, np, pp, grid, runs):
    coeffs, center, radius, inside = pp.sparse_quadratic(grid, 0.1, 0.05)
    N, columns, nodes = coeffs[0].shape[0], 24, 16

    def fpm():
        f = fk.feastinit()
        f[8], f[4], f[3] = nodes, 20, 10
        return f

    def run(name):
        eng.synchronize()
        t0 = time.perf_counter()
        if name == "polynomial":
            r = fk.feast_polynomial(coeffs, center, radius, M0=columns, fpm=fpm(), engine=eng, solver="sparse_direct", method="projected")
        else:
            r = fk.feast_nonlinear([(A, k) for k, A in enumerate(coeffs)], center, radius, M0=columns, fpm=fpm(), engine=eng, solver="sparse_direct")
        eng.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    names = ("polynomial", "nonlinear")
    for name in names:
        run(name)
    ms, last = {n: [] for n in names}, {}
    for _ in range(runs):
        for name in names:
            last[name], t = run(name)
            ms[name].append(t)
    for name in names:
        r = last[name]
        st = r.stats["polynomial" if name == "polynomial" else "nonlinear"]
        row = {"measurement": "b", "method": name, "grid": list(grid), "N": N, "columns": columns, "nodes": nodes, "ms_median": float(np.median(ms[name])),
               "ms_all": [round(t, 1) for t in ms[name]], "loops": r.loop, "M": r.M, "expected_M": len(inside), "info": r.info, "epsout": r.epsout,
               "factorizations": r.stats.get("factorizations"), "eigenvalue_error": pp.match_error(r.lambda_, inside), "plan": st.get("plan"),
               "solve_seconds": r.stats.get("solve_seconds"), "eps_history": [float(e) for e in st["eps_history"]], "rank": st["rank"],
               "candidates": st["candidates"]}
        if name == "nonlinear":
            row["host_reduced_ms"] = 1e3 * st["reduced_seconds"]
        print(json.dumps(row), flush=True)
    for name in names:
        print(json.dumps({"measurement": "b", "method": name, "classes": profiled(eng, lambda: run(name))}), flush=True)


def delay_problem(np, grid):
    """the delay problem of measurement (c) -> (terms, center, radius, eigenvalues inside, N)"""
    import scipy.sparse as sp
    from scipy.special import lambertw
    from feastkit_jl_amd import workloads
    A, B, mu = workloads.laplacian_3d_pencil(*grid)
    c, tau = -0.5, 1.0
    roots = np.concatenate([mu + lambertw(tau * c * np.exp(-tau * mu), b) / tau for b in (-1, 0, 1)])
    roots = roots[np.isfinite(roots)]
    low = roots[np.argsort(roots.real)]
    center = complex(np.mean(low[:8]))
    dist = np.sort(np.abs(roots - center))
    j = 7 + int(np.argmax(dist[8:17] - dist[7:16]))
    radius = float(0.5 * (dist[j] + dist[j + 1]))
    inside = roots[np.abs(roots - center) <= radius]
    terms = [(sp.csr_matrix(A), 0), (sp.csr_matrix(B), lambda z: -z), (sp.csr_matrix(c * B), lambda z: np.exp(-tau * z))]
    return terms, center, radius, inside, A.shape[0]


def delay_run(eng, fk, np, pp, grid, runs):
    terms, center, radius, inside, N = delay_problem(np, grid)
    fpm = fk.feastinit()
    fpm[8], fpm[3] = 16, 10
    ms = []
    for _ in range(runs + 1):
        eng.synchronize()
        t0 = time.perf_counter()
        r = fk.feast_nonlinear(terms, center, radius, M0=max(6, int(1.5 * len(inside)) + 2), fpm=fpm.copy(), engine=eng, solver="sparse_direct")
        eng.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    st = r.stats["nonlinear"]
    print(json.dumps({"measurement": "c", "grid": list(grid), "N": N, "center": [center.real, center.imag], "radius": radius,
                      "expected_M": len(inside), "M": r.M, "info": r.info, "loops": r.loop, "epsout": r.epsout, "ms_median": float(np.median(ms[1:])),
                      "ms_all": [round(t, 1) for t in ms[1:]], "host_reduced_ms": 1e3 * st["reduced_seconds"], "plan": st.get("plan"),
                      "eigenvalue_error": pp.match_error(r.lambda_, inside), "eps_history": [float(e) for e in st["eps_history"]],
                      "rank": st["rank"], "candidates": st["candidates"], "factorizations": r.stats["factorizations"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=24)
    ap.add_argument("--grid", type=int, nargs=3, default=(50, 40, 25))
    ap.add_argument("--skip", nargs="*", default=(), choices=("a", "b", "c"))
    a = ap.parse_args()
    import numpy as np
    import feastkit_jl_amd as fk
    import polynomial_probe as pp
    eng = fk.HipEngine(0)
    if "a" not in a.skip:
        form_kernels(eng, fk, np, a.N, a.nodes)
    if "b" not in a.skip:
        sparse_runs(eng, fk, np, pp, tuple(a.grid), a.runs)
    if "c" not in a.skip:
        delay_run(eng, fk, np, pp, tuple(a.grid), a.runs)
    eng.close()


if __name__ == "__main__":
    main()
