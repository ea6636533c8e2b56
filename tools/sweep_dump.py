"""Contour-sweep dump: a fixed list of contour_apply calls on one build of libfeasthip.so, every result written to an .npz, so
that two builds (a refactor and its parent) can be compared bit for bit on the CPU.

  python tools/sweep_dump.py LIB OUT.npz          run the list on the library at LIB (one child process per group)
  python tools/sweep_dump.py --compare A.npz B.npz [--self A2.npz]
      print one line per case: equal in every array, or the largest difference.  With --self (a second run of A's build):
      cases in which that build differs from itself are named, and compared within the solver's TOLERANCES entry instead.

The list covers every solver kind (LU with 64- and 32-bit factors, banded, BiCGStab, COCG fused and five-launch, shifted COCG,
block COCG with B given and B = I, GMRES), the COCG starts (zero guess, Ritz warm start, lazy start on and off, sum mode on and off) and the call variants (a
column mask, a node list with direct nodes, moments, a width above 64).  Switches that the library reads once per process
or per handle (FH_COCG_FUSED, FH_NO_SUM_MODE) get a group, that is a fresh child process, of their own; the parent process
never opens the GPU.  Per case: Q_proj, the node statuses, last_node_iterations, last_column_iterations, the stats counters
(and the moment matrices where requested).  stats.spmm_calls of the per-node Krylov sweeps counts QUEUED steps, which depends
on host polling: it is stored as `spmm_calls_queued` and left out of the comparison (the shifted sweep's is device-side)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROUPS = {"default": {}, "five_launch": {"FH_COCG_FUSED": "0"}, "no_sum_mode": {"FH_NO_SUM_MODE": "1"}}
GROUP_TIMEOUT = 240          # seconds per child process
# Relative difference allowed in a case whose own build differs from itself between two runs: what the GPU test of that solver
# allows the sweep.  LU, banded, GMRES: 1e-10 (test_gpu_primitives.py, test_gpu_banded.py, test_gpu_node_solver.py against the
# oracle's sum).  COCG, BiCGStab, shifted COCG: 64 eps, the floor of krylov_reference.tolerance (test_gpu_krylov_steps.py; its
# measured part, 32 times the drift of the restatement, is not known here, so the bound is never wider than the test's).
TOLERANCES = (("lu", 1e-10), ("banded", 1e-10), ("gmres", 1e-10), ("", 64 * np.finfo(np.float64).eps))


def tolerance(case):
    name = case.split("/", 1)[1]
    return next(tol for prefix, tol in TOLERANCES if name.startswith(prefix))


def run_group(lib_path, group, out):
    import feastkit_jl_amd as fk
    from feastkit_jl_amd import _lib
    _lib._lib = _lib.load_library(lib_path)          # every HipEngine of this process binds to this build
    eng = fk.HipEngine(0)
    data = {}

    A, lam = fk.workloads.laplacian_3d_standard(12, 10, 8)
    Ag, Bg, lamg = fk.workloads.laplacian_3d_pencil(12, 10, 8)
    N = A.shape[0]
    n = 96
    T = np.diag(2.0 * np.ones(n)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    fpm = fk.feastinit()
    fpm[2], fpm[16], fpm[18] = 8, 0, 100
    Z, W = fk.contour.feast_contour(0.0, 0.62, fpm)
    Zd, Wd = fk.contour.feast_contour(0.5, 1.5, fpm)
    # block COCG: the N = 3200 pencil and interval of tests/block_cocg_cases.py, its B = I counterpart, the test's narrow block
    Ab, Bb, lamb = fk.workloads.laplacian_3d_pencil(20, 16, 10)[:3]
    Abi, lambi = fk.workloads.laplacian_3d_standard(20, 16, 10)[:2]
    Zb, Wb = fk.contour.feast_contour(0.0, 0.42, fpm)

    def ritz(values, m):                               # Ritz values of a warm start: the spectrum's low end, perturbed
        return np.sort(values)[:m] * (1.0 + 1e-3 * np.cos(np.arange(m)))

    def case(name, problem, m, solver, warm=False, real=True, env=None, mask=None, node_list=None, direct_nodes=None,
             moments=False, contour=(Z, W), **solver_kw):
        if group != "default" and solver not in ("cocg", "shifted_cocg"):
            return
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            Ap, Bp, lp = problem
            eng.set_problem(Ap, Bp)
            eng.set_contour(contour[0], contour[1], 2.0)
            eng.set_real_projection(real)
            eng.set_node_list(np.arange(len(contour[0])) if node_list is None else node_list)
            kinds = None
            if direct_nodes is not None:
                kinds = np.zeros(len(contour[0]), dtype=np.int32)
                kinds[direct_nodes] = 4
            eng.set_node_solver(kinds)
            eng.set_solver(solver, **solver_kw)
            eng.set_column_mask(mask)
            nodes = len(contour[0]) if node_list is None else len(node_list)
            Q = fk.seeded_subspace(Ap.shape[0], m)
            res = eng.contour_apply(eng.upload(Q), m, ritz(lp, m) if warm else None, want_moments=moments)
            dP, status, st = res[:3]
            pre = group + "/" + name + "/"
            data[pre + "Q_proj"] = eng.download(dP, m)
            data[pre + "status"] = np.array(status[:nodes])
            data[pre + "node_iterations"] = eng.last_node_iterations(nodes)
            data[pre + "column_iterations"] = eng.last_column_iterations(nodes, m)
            used, seed, seed_its, _ = eng.last_shifted_sweep()
            if solver == "block_cocg":
                data[pre + "block_sweep"] = np.array(eng.last_block_sweep(), dtype=np.int64)      # used, steps, breakdowns, passes
            counters = {k: st[k] for k in ("krylov_iterations", "factorizations", "max_rel_residual")}
            counters["spmm_calls" if used or solver in ("gmres", "direct", "banded") else "spmm_calls_queued"] = st["spmm_calls"]
            counters["shifted_used"], counters["shifted_seed"], counters["shifted_seed_iterations"] = int(used), seed, seed_its
            for k, v in counters.items():
                data[pre + "stats." + k] = np.array(v)
            if moments:
                data[pre + "zAq"], data[pre + "zSq"] = res[3], res[4]
            print("%s status=%s iterations=%d%s" % (pre[:-1], list(status[:nodes]), st["krylov_iterations"],
                                                    " block_sweep=%s" % (eng.last_block_sweep(),) if solver == "block_cocg" else ""), flush=True)
        finally:
            for k in (env or {}):
                del os.environ[k]
            eng.set_column_mask(None)
            eng.set_node_solver(None)

    std, gen, dense = (A, None, lam), (Ag, Bg, lamg), (T, None, np.linalg.eigvalsh(T))
    tight = dict(rtol=1e-10, atol=0.0, maxit=400)
    loose = dict(rtol=3e-2, atol=0.0, maxit=50)          # inexact sweep: the predicted stop of the fused iteration
    mask24 = (np.arange(24) % 3 != 1).astype(np.int32)
    mask80 = (np.arange(80) % 5 != 2).astype(np.int32)
    nolazy = {"FH_NO_LAZY_START": "1"}
    case("lu64", dense, 30, "direct", contour=(Zd, Wd))
    case("lu32", dense, 30, "direct", contour=(Zd, Wd), rtol=1e-12, factor_precision=32)
    case("lu64_wide_moments", dense, 80, "direct", contour=(Zd, Wd), moments=True, real=False)
    case("banded", gen, 24, "banded")
    case("banded32", gen, 24, "banded", rtol=1e-12, factor_precision=32)
    case("bicgstab_zero", gen, 24, "bicgstab", **tight)
    case("bicgstab_ritz_mask", gen, 24, "bicgstab", warm=True, mask=mask24, **tight)
    case("bicgstab_mixed32", gen, 24, "bicgstab", warm=True, factor_precision=32, rtol=1e-5, atol=0.0, maxit=400)
    case("bicgstab_capped", gen, 24, "bicgstab", rtol=1e-12, atol=0.0, maxit=7)
    case("gmres_zero", gen, 24, "gmres", restart=20, rtol=1e-8, atol=0.0, maxit=300)
    case("gmres_ritz_mask", gen, 24, "gmres", warm=True, mask=mask24, restart=20, rtol=1e-8, atol=0.0, maxit=300)
    case("gmres_capped", gen, 24, "gmres", restart=10, rtol=1e-12, atol=0.0, maxit=12)
    for tag, prob in (("std", std), ("gen", gen)):
        case("cocg_%s_zero" % tag, prob, 24, "cocg", **tight)
        case("cocg_%s_ritz" % tag, prob, 24, "cocg", warm=True, **tight)
        case("cocg_%s_zero_nolazy" % tag, prob, 24, "cocg", env=nolazy, **tight)
        case("cocg_%s_ritz_nolazy" % tag, prob, 24, "cocg", warm=True, env=nolazy, **tight)
        case("cocg_%s_ritz_noshared" % tag, prob, 24, "cocg", warm=True, env={"FH_NO_SHARED_START": "1"}, **tight)
        case("cocg_%s_inexact" % tag, prob, 24, "cocg", warm=True, **loose)
        case("cocg_%s_capped" % tag, prob, 24, "cocg", rtol=1e-12, atol=0.0, maxit=9)
        case("cocg_%s_ritz_mask" % tag, prob, 24, "cocg", warm=True, mask=mask24, **tight)
        case("cocg_%s_moments" % tag, prob, 24, "cocg", warm=True, moments=True, real=False, **tight)
        case("cocg_%s_mixed32" % tag, prob, 24, "cocg", warm=True, factor_precision=32, rtol=1e-5, atol=0.0, maxit=400)
        case("cocg_%s_wide_mask" % tag, prob, 80, "cocg", warm=True, mask=mask80, **tight)
        case("cocg_%s_wide_moments" % tag, prob, 80, "cocg", moments=True, real=False, **tight)
        case("cocg_%s_node_list_direct" % tag, prob, 24, "cocg", warm=True, node_list=np.array([1, 2, 4, 5, 7]),
             direct_nodes=[2, 7], **tight)
        case("cocg_%s_complex_weights" % tag, prob, 24, "cocg", real=False, **tight)
    case("shifted_zero", std, 24, "shifted_cocg", **tight)
    case("shifted_ritz", std, 24, "shifted_cocg", warm=True, **tight)
    case("shifted_inexact", std, 24, "shifted_cocg", warm=True, **loose)
    case("shifted_capped", std, 24, "shifted_cocg", rtol=1e-12, atol=0.0, maxit=9)
    case("shifted_ritz_mask", std, 24, "shifted_cocg", warm=True, mask=mask24, **tight)
    case("shifted_wide_mask", std, 80, "shifted_cocg", warm=True, mask=mask80, **tight)
    case("shifted_falls_back_gen", gen, 24, "shifted_cocg", warm=True, **tight)
    case("block_cocg_gen", (Ab, Bb, lamb), 5, "block_cocg", real=False, contour=(Zb, Wb), **loose)
    case("block_cocg_std", (Abi, None, lambi), 5, "block_cocg", real=False, contour=(Zb, Wb), **loose)
    eng.close()
    np.savez(out, **data)


def dump(lib_path, out):
    merged = {}
    for group, env in GROUPS.items():
        part = "%s.%s.npz" % (out, group)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group, os.path.abspath(lib_path), part],
                            env=dict(os.environ, **env), timeout=GROUP_TIMEOUT).returncode
        if rc != 0:
            sys.exit("group %s failed with exit status %d: stopping" % (group, rc))       # nothing more is started
        with np.load(part) as z:
            merged.update({k: z[k] for k in z.files})
        os.remove(part)
    np.savez(out, **merged)
    print("wrote %s: %d cases" % (out, len({k.rsplit("/", 1)[0] for k in merged})))


def case_diff(a, b, case, keys):
    """(bitwise equal, largest relative difference over the case's arrays)"""
    worst, same = 0.0, True
    for k in keys:
        x, y = a[k], b[k]
        if x.shape == y.shape and x.tobytes() == y.tobytes():
            continue
        same = False
        if x.shape != y.shape:
            return False, float("inf")
        scale = max(float(np.abs(x).max()), 1e-300) if x.size else 1.0
        diff = float(np.abs(x.astype(np.complex128) - y.astype(np.complex128)).max()) / scale
        if not np.isfinite(diff):                          # a NaN or an infinity on one side only is never "close"
            return False, float("inf")
        worst = max(worst, diff)
    return same, worst


def compare(path_a, path_b, path_self):
    a, b = np.load(path_a), np.load(path_b)
    a2 = np.load(path_self) if path_self else None
    if sorted(a.files) != sorted(b.files):
        sys.exit("the two dumps hold different arrays: %s" % sorted(set(a.files) ^ set(b.files)))
    cases = sorted({k.rsplit("/", 1)[0] for k in a.files})
    bad = 0
    for c in cases:
        keys = [k for k in a.files if k.rsplit("/", 1)[0] == c and not k.endswith("spmm_calls_queued")]
        stable = True if a2 is None else case_diff(a, a2, c, keys)[0]
        same, worst = case_diff(a, b, c, keys)
        if same:
            verdict = "equal (bitwise, %d arrays)" % len(keys)
        elif not stable and worst <= tolerance(c):
            verdict = "A differs from itself between runs; A vs B within %.1e: max rel diff %.3e" % (tolerance(c), worst)
        else:
            verdict = "DIFFERENT: max rel diff %.3e%s" % (worst, "" if stable else " (A also differs from itself)")
            bad += 1
        print("%-44s %s" % (c, verdict))
    print("%d cases, %d different" % (len(cases), bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", default=None, help="(internal) run one group in this process")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--self", dest="self_run", default=None)
    ap.add_argument("first")
    ap.add_argument("second")
    args = ap.parse_args()
    if args.compare:
        compare(args.first, args.second, args.self_run)
    elif args.group:
        run_group(args.first, args.group, args.second)
    else:
        dump(args.first, args.second)
