"""Measurements for the count estimate of feast_polynomial / feast_nonlinear; needs the GPU.  One JSON
line per measurement.

(a) k_node_combine (profile class node_combine) inside one estimate on the N = 50 000 sparse quadratic of tools/polynomial_probe.py,
    64 columns, 16 nodes, 2 kept terms: ne + nt' panels of N x 64 complex128 moved per launch, against a device-to-device copy of
    the same byte count timed in the same run.
(b) k_spmm_fanin_trace (class fanin_trace) of the same estimate against nt' single products on the same pattern (class poly_spmm,
    one k_spmm_fan launch with one output, through poly_matmul), per launch.
(c) the whole estimate (engine.poly_estimate_count, factors cached) against one plain residual-inverse sweep of the same width
    on the same cached factors (engine.poly_resinv_apply), wall time, median of --runs, and the device time per class of one more.
(d) M0 = "auto" against the same solve with the hand-picked M0, alternating, median of --runs: feast_polynomial(method="projected",
    solver="sparse_direct") on the quadratic, feast_nonlinear(solver="sparse_direct") on the delay problem of
    tools/nonlinear_probe.py (c).

    python tools/count_probe.py [--runs 5] [--grid 50 40 25] [--skip a c d]      ((b) comes with (a))"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

CLASSES = ("node_combine", "fanin_trace", "poly_spmm", "poly_resinv", "mf_assemble", "poly_mf_assemble", "terms_mf_assemble", "lu_panel", "lu_gemm",
           "lu_gemm_in", "lu_trsm")


def profiled(eng, call):
    eng.profile_enable(True)
    eng.profile_set_period(1)
    eng.profile_reset()
    call()
    out = {}
    for cls in CLASSES:
        total, n = eng.profile_get(cls)
        if n:
            out[cls] = {"ms": round(total, 4), "launches": n}
    eng.profile_enable(False)
    return out


def median_ms(eng, np, call, runs):
    ms = []
    for _ in range(runs + 1):
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        eng.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms[1:])), [round(t, 2) for t in ms[1:]]


def kernels(eng, fk, np, pp, grid, runs, skip):
    import torch
    from feastkit_jl_amd import hip_backend as hb
    from feastkit_jl_amd.ingest import polynomial_union_csr
    coeffs, center, radius, inside = pp.sparse_quadratic(grid, 0.1, 0.05)
    N, m, nodes = coeffs[0].shape[0], 64, 16
    fpm = fk.feastinit()
    fpm[8] = nodes
    Zne, Wne = fk.feast_gcontour(center, radius, fk.feastdefault(fpm))
    eng.set_polynomial_csr(*polynomial_union_csr(coeffs))
    eng.set_solver("direct", cache_factors=True, factor_precision=64)
    eng.set_real_projection(False)
    eng.set_contour(Zne, Wne, 1.0)
    G = Wne[:, None] * hb.poly_derivative_table(2, Zne)
    kept = int(np.count_nonzero(np.abs(G).max(axis=0)))
    t, status, st = eng.poly_estimate_count(m, 1, G)                      # factors every node
    row = {"N": N, "columns": m, "nodes": nodes, "kept_terms": kept, "mean": [float(np.mean(t).real), float(np.mean(t).imag)],
           "stderr": float(np.std(t, ddof=1) / np.sqrt(m)), "inside": len(inside), "factorizations": st["factorizations"]}
    if "a" not in skip:
        prof = profiled(eng, lambda: eng.poly_estimate_count(m, 1, G))
        dX = eng.upload(np.ones((2 * N, m)) + 0j)
        prod = profiled(eng, lambda: eng.poly_matmul(1, dX, m))["poly_spmm"]
        panel = 16.0 * N * m
        traffic = panel * (nodes + kept)
        nc_ms = prof["node_combine"]["ms"] / prof["node_combine"]["launches"]
        n = int(traffic // 32)                                            # a copy that reads and writes `traffic` bytes in all
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
        del src, dst
        a = dict(row, measurement="a", bytes_per_launch=traffic, node_combine={"ms": round(nc_ms, 4), "GB_per_s": round(traffic / (nc_ms * 1e-3) / 1e9, 1)},
                 copy={"ms": round(best, 4), "GB_per_s": round(traffic / (best * 1e-3) / 1e9, 1)})
        a["node_combine"]["fraction_of_copy"] = round(best / nc_ms, 4)
        print(json.dumps(a), flush=True)
        ft_ms = prof["fanin_trace"]["ms"] / prof["fanin_trace"]["launches"]
        one = prod["ms"] / prod["launches"]
        print(json.dumps(dict(row, measurement="b", fanin_trace_ms=round(ft_ms, 4), single_product_ms=round(one, 4), single_products=kept,
                              fanin_over_products=round(ft_ms / (kept * one), 4))), flush=True)
    if "c" not in skip:
        dV = eng.upload(np.ones((N, m)) + 0j)
        est_ms, est_all = median_ms(eng, np, lambda: eng.poly_estimate_count(m, 1, G), runs)
        sw_ms, sw_all = median_ms(eng, np, lambda: eng.poly_resinv_apply(dV, m), runs)
        print(json.dumps(dict(row, measurement="c", estimate_ms=est_ms, estimate_all=est_all, sweep_ms=sw_ms, sweep_all=sw_all,
                              estimate_over_sweep=round(est_ms / sw_ms, 4), estimate_classes=profiled(eng, lambda: eng.poly_estimate_count(m, 1, G)),
                              sweep_classes=profiled(eng, lambda: eng.poly_resinv_apply(dV, m)))), flush=True)
    eng.free_factors()


def auto_runs(eng, fk, np, pp, grid, runs):
    import nonlinear_probe as npb
    coeffs, center, radius, inside = pp.sparse_quadratic(grid, 0.1, 0.05)
    terms, dcenter, dradius, dinside, _ = npb.delay_problem(np, grid)

    def fpm():
        f = fk.feastinit()
        f[8], f[4], f[3] = 16, 20, 10
        return f

    problems = {
        "quadratic": (lambda M0: fk.feast_polynomial(coeffs, center, radius, M0=M0, fpm=fpm(), engine=eng, solver="sparse_direct", method="projected"),
                      24, inside, "polynomial"),
        "delay": (lambda M0: fk.feast_nonlinear(terms, dcenter, dradius, M0=M0, fpm=fpm(), engine=eng, solver="sparse_direct"),
                  max(6, int(1.5 * len(dinside)) + 2), dinside, "nonlinear"),
    }
    for name, (solve, hand, exact, key) in problems.items():
        ms, last = {"hand": [], "auto": []}, {}
        for which in ("hand", "auto"):
            solve(hand if which == "hand" else "auto")
        for _ in range(runs):
            for which in ("hand", "auto"):
                eng.synchronize()
                t0 = time.perf_counter()
                last[which] = solve(hand if which == "hand" else "auto")
                eng.synchronize()
                ms[which].append(1e3 * (time.perf_counter() - t0))
        for which in ("hand", "auto"):
            r = last[which]
            row = {"measurement": "d", "problem": name, "M0": which, "N": r.q.shape[0], "ms_median": float(np.median(ms[which])),
                   "ms_all": [round(t, 1) for t in ms[which]], "columns": r.stats[key]["columns"], "loops": r.loop, "M": r.M, "expected_M": len(exact),
                   "info": r.info, "epsout": r.epsout, "factorizations": r.stats["factorizations"], "eigenvalue_error": pp.match_error(r.lambda_, exact)}
            if which == "auto":
                est = r.stats["estimate"]
                row.update(M0_auto=r.stats["M0_auto"], estimate_mean=[est["mean"].real, est["mean"].imag], estimate_stderr=est["stderr"],
                           estimate_ms=1e3 * est["seconds"])
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=3, default=(50, 40, 25))
    ap.add_argument("--skip", nargs="*", default=(), choices=("a", "c", "d"))
    a = ap.parse_args()
    import numpy as np
    import feastkit_jl_amd as fk
    import polynomial_probe as pp
    eng = fk.HipEngine(0)
    if not {"a", "c"} <= set(a.skip):
        kernels(eng, fk, np, pp, tuple(a.grid), a.runs, a.skip)
    if "d" not in a.skip:
        auto_runs(eng, fk, np, pp, tuple(a.grid), a.runs)
    eng.close()


if __name__ == "__main__":
    main()
