"""Measurements for operator handles; needs the GPU.  One JSON line per measurement.

(a) the combine kernel (profile class op_combine, k_op_combine) at N = 50 000, 16 nodes, ld = 64: a five-step BiCGStab sweep on
    a diagonal operator with B = I (every node stays active), GB/s on the algorithmic bytes of its launches against a
    device-to-device copy of the same byte count timed in the same run.
(b) the cfg 3 grid (50 x 40 x 25 Laplacian pencil, 8 nodes, m = 64, five-launch COCG from the zero guess): an operator handle
    whose callbacks are torch sparse products with the same matrices against the CSR handle under the same non-fused solver
    (FH_COCG_FUSED=0, set here before the library loads); milliseconds per sweep and per Krylov step, median of --runs, and the
    callback's share of the operator handle's wall time from engine.operator_stats().

--terms, term-operator handles:
(t) the term combine kernel (profile class terms_combine, k_terms_combine) on the workload of (a) as a split form of nt = 3 and
    nt = 9 terms (the identity plus nt - 1 diagonal operators), a five-step BiCGStab sweep through nep_resinv_apply: GB/s on
    the algorithmic bytes against a device-to-device copy of the same byte count; (a) runs first in the same process, so
    k_op_combine's ratio to its copy is of the same run.
(d) the delay problem of tools/nonlinear_probe.py (c) on the 50 x 40 x 25 grid, A - lambda B + c e^{-tau lambda} B with B = I +
    0.1 A, through feast_nonlinear_matvec as the two-term split form g_0(lambda) A + g_1(lambda) I on the slicing stencil of
    README.md (solver "cocg"), against feast_nonlinear(solver="sparse_direct") on the matrices in the same run: wall time, loops,
    Krylov steps, callback_seconds and the device memory held.

    python tools/operator_probe.py [--runs 5] [--skip a b] [--terms]"""
import argparse
import json
import os
import sys
import time

os.environ["FH_COCG_FUSED"] = "0"          # read once per process: both handles of (b) take the five-launch iteration
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def probe_combine(fk, eng, torch):
    import numpy as np
    N, ne, m, steps = 50_000, 16, 64, 5
    d = torch.linspace(1.0, 9.0, N, dtype=torch.float64, device=eng.device)[None, :, None]
    eng.set_operator(N, lambda Y, X: torch.mul(X, d, out=Y), None, real=True, symmetric=True, batched=True)
    fpm = fk.feastinit()
    fpm[2] = ne
    fk.feastdefault(fpm)
    eng.set_contour(*fk.feast_contour(-20.0, -10.0, fpm), 2.0)        # away from the spectrum: no column leaves in five steps
    eng.set_real_projection(True)
    eng.set_solver("bicgstab", rtol=1e-30, atol=0.0, maxit=steps)
    dQ = eng.upload(fk.seeded_subspace(N, m))
    eng.contour_apply(dQ, m)                                           # warm-up: buffers, views
    eng.profile_enable(True)
    eng.profile_set_period(1)
    eng.profile_reset()
    _, status, st = eng.contour_apply(dQ, m)
    ms, launches = eng.profile_get("op_combine")
    eng.profile_enable(False)
    P = 16 * N * 64
    # B Q is not formed (B = I); start residual: AX, X, Bvec read, Y written (4 P per node); per step V = S P with <Rhat, V>
    # (AX, X, U, Y: 4 P) and T = S S with <T, S>, <T, T> (AX, X, Y: 3 P)
    nbytes = ne * P * (4 + steps * (4 + 3))
    buf = torch.empty(nbytes // 2 // launches, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(launches):
        dst.copy_(buf)
    ev1.record()
    torch.cuda.synchronize()
    copy_ms = ev0.elapsed_time(ev1)
    print(json.dumps({"probe": "a", "N": N, "nodes": ne, "ld": 64, "launches": launches, "spmm_calls": st["spmm_calls"],
                      "node_status": [int(s) for s in status[:ne]], "algorithmic_GB": round(nbytes / 1e9, 3),
                      "op_combine_ms": round(ms, 3), "op_combine_GBps": round(nbytes / 1e6 / ms, 1),
                      "copy_ms": round(copy_ms, 3), "copy_GBps": round(nbytes / 1e6 / copy_ms, 1)}), flush=True)


def probe_sweeps(fk, eng, torch, runs):
    import numpy as np
    A, B, _ = fk.workloads.laplacian_3d_pencil(50, 40, 25)
    N, m = A.shape[0], 64
    fpm = fk.feastinit()
    fpm[2] = 8
    fk.feastdefault(fpm)
    Z, W = fk.feast_contour(0.0, 0.5, fpm)
    Q = fk.seeded_subspace(N, m)

    def csr(M):
        return torch.sparse_csr_tensor(torch.from_numpy(M.indptr.astype(np.int64)), torch.from_numpy(M.indices.astype(np.int64)),
                                       torch.from_numpy(M.data.astype(np.float64)), size=M.shape).to(eng.device)
    TA, TB = csr(A), csr(B)

    def sweep(setup):
        setup()
        eng.set_contour(Z, W, 2.0)
        eng.set_real_projection(True)
        eng.set_solver("cocg", rtol=1e-8, atol=0.0, maxit=300)
        dQ = eng.upload(Q)
        eng.contour_apply(dQ, m)                                       # warm-up
        times, st, ops = [], None, None
        for _ in range(runs):
            before = eng.operator_stats()
            t0 = time.perf_counter()
            _, status, st = eng.contour_apply(dQ, m)
            times.append(time.perf_counter() - t0)
            after = eng.operator_stats()
            ops = {k: after[k] - before[k] for k in after}
        t = median(times)
        return {"sweep_ms": round(1e3 * t, 2), "krylov_steps": int(st["spmm_calls"]), "ms_per_step": round(1e3 * t / max(1, st["spmm_calls"]), 3),
                "node_iterations_sum": int(st["krylov_iterations"]), "worst_status": int(max(status)), "operator": ops}

    out_csr = sweep(lambda: eng.set_problem(A, B))
    out_op = sweep(lambda: eng.set_operator(N, lambda Y, X: Y.copy_(torch.sparse.mm(TA, X)), lambda Y, X: Y.copy_(torch.sparse.mm(TB, X)),
                                            real=True, symmetric=True))
    share = out_op["operator"]["callback_seconds"] / (out_op["sweep_ms"] / 1e3)
    print(json.dumps({"probe": "b", "N": N, "nodes": 8, "m": m, "solver": "cocg (five-launch)", "runs": runs, "csr_handle": out_csr,
                      "operator_handle": out_op, "callback_share_of_wall": round(share, 3),
                      "operator_over_csr": round(out_op["sweep_ms"] / out_csr["sweep_ms"], 2)}), flush=True)


def probe_terms(fk, eng, torch, nt):
    import numpy as np
    N, ne, m, steps = 50_000, 16, 64, 5
    ds = [torch.linspace(1.0 + k, 9.0 + k, N, dtype=torch.float64, device=eng.device)[None, :, None] for k in range(nt)]
    muls = [None] + [(lambda Y, X, d=ds[k]: torch.mul(X, d, out=Y)) for k in range(1, nt)]
    eng.set_term_operator(N, muls, real=True, symmetric=True, batched=True)
    fpm = fk.feastinit()
    fpm[8] = ne
    fk.feastdefault(fpm)
    Z, W = fk.feast_gcontour(-15.0 + 0.0j, 5.0, fpm)                 # away from the spectrum: no column leaves in five steps
    eng.set_real_projection(False)
    eng.set_contour(Z, W, 1.0)
    F = np.stack([np.asarray(Z) if k == 0 else np.full(ne, -1.0 / nt + 0j) for k in range(nt)], axis=1)      # T(z) = z I - sum_k D_k / nt
    eng.nep_set_node_values(F)
    eng.set_solver("bicgstab", rtol=1e-30, atol=0.0, maxit=steps)
    dQ = eng.upload(fk.seeded_subspace(N, m))
    eng.nep_resinv_apply(dQ, m)                                        # warm-up: buffers, views
    eng.profile_enable(True)
    eng.profile_set_period(1)
    eng.profile_reset()
    before = eng.operator_stats()
    _, status, st = eng.nep_resinv_apply(dQ, m)
    ms, launches = eng.profile_get("terms_combine")
    eng.profile_enable(False)
    after = eng.operator_stats()
    P, ntp = 16 * N * 64, nt - 1
    # start residual: nt' products, X (the identity term), Bvec read, Y written (nt' + 3 P per node); per step V = S P with
    # <Rhat, V> (nt' products, X, U, Y: nt' + 3 P) and T = S S with <T, S>, <T, T> (nt' products, X, Y: nt' + 2 P)
    nbytes = ne * P * ((ntp + 3) + steps * ((ntp + 3) + (ntp + 2)))
    buf = torch.empty(nbytes // 2 // launches, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(launches):
        dst.copy_(buf)
    ev1.record()
    torch.cuda.synchronize()
    copy_ms = ev0.elapsed_time(ev1)
    print(json.dumps({"probe": "t", "nt": nt, "N": N, "nodes": ne, "ld": 64, "launches": launches, "spmm_calls": st["spmm_calls"],
                      "node_status": [int(s) for s in status[:ne]], "term_calls": [a - b for a, b in zip(after["term_calls"], before["term_calls"])],
                      "algorithmic_GB": round(nbytes / 1e9, 3), "terms_combine_ms": round(ms, 3),
                      "terms_combine_GBps": round(nbytes / 1e6 / ms, 1), "copy_ms": round(copy_ms, 3),
                      "copy_GBps": round(nbytes / 1e6 / copy_ms, 1), "ratio_to_copy": round(copy_ms / ms, 3)}), flush=True)
    del buf, dst


def probe_delay(fk, eng, torch, runs):
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import nonlinear_probe as nlp
    import polynomial_probe as pp
    grid = (50, 40, 25)
    terms, center, radius, inside, N = nlp.delay_problem(np, grid)
    nx, ny, nz = grid[::-1]                  # (x fastest: the panel's rows are (z, y, x))
    c, tau, shift = -0.5, 1.0, 0.1

    def laplace(Y, X):
        x, y = X.view(nx, ny, nz, -1), Y.view(nx, ny, nz, -1)
        y.copy_(x).mul_(6.0)
        y[1:].sub_(x[:-1]); y[:-1].sub_(x[1:]); y[:, 1:].sub_(x[:, :-1]); y[:, :-1].sub_(x[:, 1:])
        y[:, :, 1:].sub_(x[:, :, :-1]); y[:, :, :-1].sub_(x[:, :, 1:])
    # A - lambda (I + s A) + c e^{-tau lambda} (I + s A) = g_0 A + g_1 I
    split = [(laplace, lambda z: 1.0 - shift * z + shift * c * np.exp(-tau * z)), (None, lambda z: -z + c * np.exp(-tau * z))]
    fpm = fk.feastinit()
    fpm[8], fpm[3] = 16, 10
    M0 = max(6, int(1.5 * len(inside)) + 2)
    out = {"probe": "d", "grid": list(grid), "N": N, "expected_M": len(inside), "M0": M0}
    for name, call in (("sparse_direct", lambda: fk.feast_nonlinear(terms, center, radius, M0=M0, fpm=fpm.copy(), engine=eng, solver="sparse_direct")),
                       ("matvec_cocg", lambda: fk.feast_nonlinear_matvec(split, N, center, radius, M0=M0, fpm=fpm.copy(), engine=eng, solver="cocg",
                                                                         symmetric=True))):
        ms = []
        for _ in range(runs + 1):
            eng.synchronize()
            t0 = time.perf_counter()
            r = call()
            eng.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        free, total = torch.cuda.mem_get_info()
        rec = r.stats["nonlinear"]
        out[name] = {"ms_median": round(median(ms[1:]), 1), "M": r.M, "info": r.info, "loops": r.loop, "epsout": float(r.epsout),
                     "eigenvalue_error": float(pp.match_error(r.lambda_, inside)) if r.M == len(inside) else None,
                     "krylov_iterations": int(r.stats["krylov_iterations"]), "factorizations": int(r.stats["factorizations"]),
                     "device_GB_in_use": round((total - free) / 1e9, 2)}
        if "krylov" in rec:
            out[name]["krylov"] = [(k["iterations"], k["capped_nodes"]) for k in rec["krylov"]]
            out[name]["operator"] = {k: v for k, v in r.stats["operator"].items()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[])
    ap.add_argument("--terms", action="store_true", help="the term-operator measurements (t) and (d) after (a)")
    args = ap.parse_args()
    import torch
    import feastkit_jl_amd as fk
    eng = fk.HipEngine(0)
    if "a" not in args.skip:
        probe_combine(fk, eng, torch)
    if "b" not in args.skip and not args.terms:
        probe_sweeps(fk, eng, torch, args.runs)
    if args.terms:
        if "t" not in args.skip:
            for nt in (3, 9):
                probe_terms(fk, eng, torch, nt)
        if "d" not in args.skip:
            probe_delay(fk, eng, torch, args.runs)
    eng.close()


if __name__ == "__main__":
    main()
