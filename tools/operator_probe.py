"""Measurements for operator handles; needs the GPU.  One JSON line per measurement.

(a) the combine kernel (profile class op_combine, k_op_combine) at N = 50 000, 16 nodes, ld = 64: a five-step BiCGStab sweep on
    a diagonal operator with B = I (every node stays active), GB/s on the algorithmic bytes of its launches against a
    device-to-device copy of the same byte count timed in the same run.
(b) the cfg 3 grid (50 x 40 x 25 Laplacian pencil, 8 nodes, m = 64, five-launch COCG from the zero guess): an operator handle
    whose callbacks are torch sparse products with the same matrices against the CSR handle under the same non-fused solver
    (FH_COCG_FUSED=0, set here before the library loads); milliseconds per sweep and per Krylov step, median of --runs, and the
    callback's share of the operator handle's wall time from engine.operator_stats().

    python tools/operator_probe.py [--runs 5] [--skip a b]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[])
    args = ap.parse_args()
    import torch
    import feastkit_jl_amd as fk
    eng = fk.HipEngine(0)
    if "a" not in args.skip:
        probe_combine(fk, eng, torch)
    if "b" not in args.skip:
        probe_sweeps(fk, eng, torch, args.runs)
    eng.close()


if __name__ == "__main__":
    main()
