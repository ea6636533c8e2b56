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


CLASSES = ("poly_form", "poly_rhs", "poly_expand", "poly_residual", "lu_form", "lu_panel", "lu_laswp", "lu_trsm", "lu_gemm_in", "lu_gemm",
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
    a = ap.parse_args()
    sys.path[:0] = [a.package_root]
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
        if name == "polynomial":
            r = fk.feast_polynomial(coeffs, center, radius, M0=a.M0, fpm=fpm(), engine=eng, Q0=Q0, residual="reference")
        else:
            r = fk.feast_general(Alin, Blin, center, radius, M0=a.M0 * d, fpm=fpm(), engine=eng, Q0=Q0)
        eng.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    names = ("companion",) if a.companion_only else ("polynomial", "companion")
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
        if name == "polynomial":
            row["backward_error_max"] = float(np.max(r.stats["polynomial"]["backward_error"]))
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
    eng.close()


def N2(name, N, d):
    return float(N if name == "polynomial" else d * N) ** 2


if __name__ == "__main__":
    main()
