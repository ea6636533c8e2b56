"""Krylov solves on P(z) for sparse coefficients (feast_polynomial(..., solver="bicgstab" | "cocg" | "gmres")): the operator
of the device restated for the step-exact references, the inexact projected driver, and the cases of
test_polynomial_krylov_host.py / test_gpu_polynomial_krylov.py with their reference results (cached per process).

PolyOp stands where krylov_reference.Pencil stands: krylov_reference.solve_column and gmres_reference.solve_batch reach their
operator through ``apply(z, x)``, ``dtype``, ``real`` and ``N`` only.  PolyOp.apply restates csrc/fh_poly.hip: k_spmm_poly --
the values of every coefficient on ingest.polynomial_union_csr's pattern (explicit zeros included), per nonzero
s = sum_k a_k z^k by Horner from a_d down, the row sum in CSR order.  COCG on a polynomial handle runs the five-launch form,
so its restatement is "cocg5".

inexact_driver is polynomial_projected_reference.driver with every numpy.linalg.solve replaced by per-column reference
solves from a zero start without a preconditioner (relative stop test); both files are imported, neither is changed."""
import functools
import math

import numpy as np
import scipy.linalg as sla

import feast_oracle as fo
import gmres_reference as gr
import krylov_cases as kc
import krylov_reference as kr
import polynomial_projected_reference as ppr
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd.ingest import polynomial_union_csr
from test_gpu_primitives import rand_block

MARGIN_MIN, LEFT_OUT_MAX, POWER = kc.MARGIN_MIN, kc.LEFT_OUT_MAX, kc.POWER


class PolyOp:
    """S(z) x = P(z) x in the arithmetic of ``dtype``, as k_spmm_poly forms it."""

    def __init__(self, coeffs, dtype=np.clongdouble):
        self.dtype = np.dtype(dtype)
        self.real = np.zeros(1, self.dtype).real.dtype
        rowptr, col, vals = polynomial_union_csr(coeffs)
        self.N = len(rowptr) - 1
        assert (np.diff(rowptr) > 0).all()              # the union pattern holds the diagonal: the row sum needs an entry per row
        cplx = np.iscomplexobj(vals[0])
        self.vals = [v.astype(self.dtype if cplx else self.real) for v in vals]
        self.col = np.asarray(col)
        self.ptr = np.asarray(rowptr[:-1])

    def apply(self, z, x):
        z = self.dtype.type(z)
        s = np.zeros(len(self.col), self.dtype)
        for v in reversed(self.vals):                   # Horner per nonzero, from a_d down
            s = s * z + v
        return np.add.reduceat(s * np.asarray(x)[self.col], self.ptr)


def dense_poly(coeffs, z, dtype=np.clongdouble):
    """P(z) as a dense matrix in ``dtype`` (plain linear algebra, for the checks of the restatement itself)."""
    ct = np.dtype(dtype)
    P = np.zeros(coeffs[0].shape, ct)
    for k, c in enumerate(coeffs):
        P = P + np.asarray(c.toarray() if hasattr(c, "toarray") else c).astype(ct) * ct.type(z) ** k
    return P


# ---- the inexact projected driver --------------------------------------------------------------------------------------------
def inexact_sweep(op, coeffs, Zne, Wne, X, sigma, method, rtol, maxit, counts=None):
    """ppr.sweep with Y_e = P(z_e)^-1 R replaced by per-column solves (kr.solve_column, zero start, atol = 0) in complex128.
    counts (a list): gets (steps[node][col], capped nodes) of the sweep."""
    X = np.asarray(X, dtype=np.complex128)
    Q = np.zeros_like(X)
    R = X if sigma is None else ppr.eval_cols(coeffs, sigma, X)
    steps, capped = [], 0
    for z, w in zip(Zne, Wne):
        cols = [kr.solve_column(op, z, R[:, j], method, rtol, 0.0, maxit) for j in range(X.shape[1])]
        Y = np.stack([c.x for c in cols], axis=1).astype(np.complex128)
        steps.append([c.steps for c in cols])
        capped += int(kr.node_status(cols, rtol, 0.0) != 0)
        Q += w * Y if sigma is None else (w / (z - np.asarray(sigma)))[None, :] * (X - Y)
    if counts is not None:
        counts.append((np.array(steps), capped))
    return Q


def inexact_driver(sparse_coeffs, center, radius, m0, method, rtol, maxit=2000, ne=sc.NE, fpm3=sc.FPM3, fpm4=20, seed=20260515,
                   perturb=0.0):
    """The loop of ppr.driver (same start block, orthonormalisation, selection) on inexact sweeps -> its dict plus
    krylov = [{iterations, node_iterations, capped_nodes} per loop]."""
    coeffs = sc.dense(sparse_coeffs)
    op = PolyOp(sparse_coeffs, np.complex128)
    d, N = len(coeffs) - 1, coeffs[0].shape[0]
    Zne, Wne = fo.feast_gcontour(center, radius, ne)
    X = fo.seeded_subspace(N, m0, seed)
    if perturb:
        X = X * (1.0 + perturb * np.random.default_rng(99).standard_normal(X.shape))
    sigma, tol, loop = None, 10.0 ** -fpm3, 0
    hist, kry = [], []
    while True:
        counts = []
        Q = inexact_sweep(op, coeffs, Zne, Wne, X, sigma, method, rtol, maxit, counts)
        steps, capped = counts[0]
        kry.append({"iterations": int(steps.max()), "node_iterations": [int(v) for v in steps.max(axis=1)], "capped_nodes": capped})
        nrm = np.linalg.norm(Q, axis=0)
        Q = Q / np.where(nrm > 0, nrm, 1.0)
        Q, r = fo.qr_compress(Q, Q.shape[1], ppr.RANK_TOL)
        theta, V = sla.eig(*pr.companion([Q.conj().T @ (Ak @ Q) for Ak in coeffs]))
        Xc = Q @ V[:r, :]
        cn = np.linalg.norm(Xc, axis=0)
        Xc = Xc / np.where(cn > 0, cn, 1.0)
        be = ppr.candidate_errors(coeffs, theta, Xc)
        be[~(cn > 0)] = np.inf
        sel, good, _ = ppr.select(theta, be, center, radius, min(m0, d * r))
        M = int(good.sum())
        epsout = float(be[sel][good].max()) if M else math.inf
        hist.append(epsout)
        if (M and epsout <= tol) or loop >= fpm4:
            idx = sel[good]
            idx = idx[np.argsort(np.abs(theta[idx]) ** 2, kind="stable")]
            return {"info": 0 if (M and epsout <= tol) else 2, "M": M, "lam": theta[idx], "q": Xc[:, idx], "epsout": epsout,
                    "loop": loop, "eps_history": hist, "krylov": kry}
        X = Xc[:, sel]
        sigma = np.where(np.isfinite(theta[sel]), theta[sel], center)
        loop += 1


# the pinned inexact runs: (name, scaled, method of the restatement, device solver, solver_tol); columns / seed / loop: ppr.DAMPED_PINS
INEXACT_PINS = (("20x16", False, "bicgstab", "bicgstab", 1e-4), ("20x16", False, "cocg5", "cocg", 1e-4),
                ("24x18", True, "bicgstab", "bicgstab", 1e-4))
INEXACT_IDS = ["20x16-bicgstab", "20x16-cocg", "24x18-scaled-bicgstab"]
HISTORY_FACTOR = 1.5        # every history entry within this factor of the exact-solve restatement's


@functools.lru_cache(maxsize=None)
def inexact_run(name, scaled, method, rtol, perturb=0.0, maxit=2000):
    columns, seed, _ = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    return inexact_driver(case["coeffs"], case["center"], case["radius"], columns, method, rtol, maxit=maxit, seed=seed, perturb=perturb)


# ---- single-shift cases ------------------------------------------------------------------------------------------------------
FAR_Z = sc.CENTER + sc.RADIUS * np.exp(0.7j)          # far from the spectrum of mixed_pattern_coeffs
MIXED = tuple((g, d, c) for g in sc.GRIDS for d, c in ((2, False), (3, True)))


def damped_shift(node):
    case = sc.damped_case("20x16", False)
    Z, _ = fo.feast_gcontour(case["center"], case["radius"], sc.NE)
    return complex(Z[node])


def _operator(key):
    """key: ("mixed", grid, d, cplx) | ("damped", node) -> (sparse coefficients, shift)"""
    if key[0] == "mixed":
        return sc.mixed_pattern_coeffs(key[1], key[2], key[3]), complex(FAR_Z)
    return sc.damped_case("20x16", False)["coeffs"], damped_shift(key[1])


# rows a, b, c of the case table: (restatement, device solver, operator keys, cuts).  BiCGStab on the damped operator next to
# the spectrum: from k = 15 on the drift of the restatement itself passes the discriminating power, so its cuts end at 5.
# Row f: N = 4200 under 40 columns (64-lane row slices, 4 rows per workgroup pass): more rows than the 1024 workgroups of
# k_spmm_poly's grid take in one pass, so a thread adds several rows into its partial sums.
BIG = ("mixed", (70, 60, 1), 2, False)
TRUNC = {
    "a-mixed-bicgstab": ("bicgstab", "bicgstab", tuple(("mixed",) + m for m in MIXED), (1, 2, 3, 5, 15, 16, 17), 6),
    "b-damped-cocg": ("cocg5", "cocg", (("damped", 0), ("damped", 5)), (1, 2, 3, 5, 15, 16, 17, 31, 33, 48), 6),
    "c-damped-bicgstab": ("bicgstab", "bicgstab", (("damped", 0), ("damped", 5)), (1, 2, 3, 5), 6),
    "f-grid-stride-bicgstab": ("bicgstab", "bicgstab", (BIG,), (1, 3), 40),
    "f-grid-stride-cocg": ("cocg5", "cocg", (BIG,), (2,), 40),
}
TRUNC_PARAMS = [(row, key) for row, v in TRUNC.items() for key in v[2]]
# rows d, e: own stop step at these tolerances, maxit 400
STOP = {
    "d-damped-cocg": ("cocg5", "cocg", (("damped", 0), ("damped", 5))),
    "e-mixed-bicgstab": ("bicgstab", "bicgstab", tuple(("mixed",) + m for m in MIXED)),
}
STOP_RTOLS = (3e-2, 1e-4)
STOP_MAXIT = 400
STOP_PARAMS = [(row, key, rtol) for row, v in STOP.items() for key in v[2] for rtol in STOP_RTOLS]


def case_id(p):
    """pytest id of one parameter value (nested tuples flattened)"""
    if isinstance(p, tuple):
        return "-".join(case_id(x) for x in p)
    return str(p)


class Case:
    pass


def stop_block(coeffs, mixed):
    """Twelve random columns scaled 1e-3 .. 1e3; for the mixed operators (whose random columns all stop at step 2 or 5) also six
    columns of mixed spectral content as krylov_cases.stop_inputs has them: sums of 1, 2, 4, ... eigenvectors of the symmetric
    A_0 = L + 4 I under scales 1e-2 .. 1e3."""
    N = coeffs[0].shape[0]
    rng = np.random.default_rng([20260720, N])
    X = (rng.standard_normal((N, 12)) + 1j * rng.standard_normal((N, 12))) * 10.0 ** np.linspace(-3.0, 3.0, 12)[None, :]
    if mixed:
        _, V = sla.eigh(coeffs[0].toarray().real)
        extra = []
        for j in range(6):
            n = min(2 ** j, N)
            pick = rng.choice(N, size=n, replace=False)
            extra.append(10.0 ** (j - 2.0) * (V[:, pick] @ rng.uniform(0.5, 1.5, size=n)))
        X = np.concatenate([X, np.array(extra).T.astype(np.complex128)], axis=1)
    return np.asfortranarray(X)


@functools.lru_cache(maxsize=None)
def trunc_case(row, key):
    """Reference columns run once to max(ks) with their history; per k the drift (krylov_cases.trunc_case on a PolyOp)."""
    method, solver, _, ks, m = TRUNC[row]
    coeffs, z = _operator(key)
    c = Case()
    c.coeffs, c.z, c.ks, c.solver, c.m = coeffs, z, ks, solver, m
    c.N = coeffs[0].shape[0]
    c.X = rand_block(c.N, m, 8)
    kmax = max(ks)
    PL, PD = PolyOp(coeffs, np.clongdouble), PolyOp(coeffs, np.complex128)
    c.ref = [kr.solve_column(PL, z, c.X[:, j], method, 1e-14, 0.0, kmax, keep_history=True) for j in range(c.m)]
    c.drift = {k: 0.0 for k in ks}
    for chunks, seed in kr.DRIFT_ORDERS:
        dots = kr.Dots(c.N, chunks, seed)
        for j, ref in enumerate(c.ref):
            dd = kr.solve_column(PD, z, c.X[:, j], method, 1e-14, 0.0, kmax, dots=dots, keep_history=True)
            for k in ks:
                xr, sr = kr.truncated(ref, k)[:2]
                xd, sd = kr.truncated(dd, k)[:2]
                if sr == sd:
                    c.drift[k] = max(c.drift[k], kr.rel_dist(xd, xr))
    return c


@functools.lru_cache(maxsize=None)
def stop_case(row, key, rtol):
    """krylov_cases.stop_case on a PolyOp: every column to its own stop step."""
    method, solver, _ = STOP[row]
    coeffs, z = _operator(key)
    c = Case()
    c.coeffs, c.z, c.solver, c.rtol = coeffs, z, solver, rtol
    c.N = coeffs[0].shape[0]
    c.X = stop_block(coeffs, key[0] == "mixed")
    c.m = c.X.shape[1]
    PL, PD = PolyOp(coeffs, np.clongdouble), PolyOp(coeffs, np.complex128)
    c.ref = [kr.solve_column(PL, z, c.X[:, j], method, rtol, 0.0, STOP_MAXIT) for j in range(c.m)]
    c.decided = np.array([r.margin >= MARGIN_MIN for r in c.ref])
    c.drift = np.zeros(c.m)
    c.fp64_steps_agree = True
    for chunks, seed in kr.DRIFT_ORDERS:
        dots = kr.Dots(c.N, chunks, seed)
        for j in range(c.m):
            dd = kr.solve_column(PD, z, c.X[:, j], method, rtol, 0.0, STOP_MAXIT, dots=dots)
            if c.decided[j]:
                c.fp64_steps_agree &= dd.steps == c.ref[j].steps
                c.drift[j] = max(c.drift[j], kr.rel_dist(dd.x, c.ref[j].x))
    return c


# GMRES on the N = 286 mixed quadratic: one node, restart 8, cuts inside a cycle, on its boundary and a step after it
GMRES_KEY, GMRES_RESTART, GMRES_KS = ("mixed", sc.GRIDS[1], 2, False), 8, (5, 8, 9)


@functools.lru_cache(maxsize=None)
def gmres_case():
    coeffs, z = _operator(GMRES_KEY)
    c = Case()
    c.coeffs, c.z, c.ks, c.restart, c.m = coeffs, z, GMRES_KS, GMRES_RESTART, 6
    c.N = coeffs[0].shape[0]
    c.X = rand_block(c.N, 6, 8)
    kmax, keep = max(c.ks), set(c.ks)
    c.batch = gr.solve_batch(PolyOp(coeffs, np.clongdouble), [z], c.X, None, 1e-14, 0.0, kmax, c.restart, keep_history=keep)
    c.want = {k: [gr.truncated(c.batch, r, k) for r in c.batch.cols[0]] for k in c.ks}
    c.products = {k: gr.truncated_products(c.batch, k) for k in c.ks}
    c.drift = {k: 0.0 for k in c.ks}
    PD = PolyOp(coeffs, np.complex128)
    for chunks, seed in kr.DRIFT_ORDERS:
        d = gr.solve_batch(PD, [z], c.X, None, 1e-14, 0.0, kmax, c.restart, dots=kr.Dots(c.N, chunks, seed), keep_history=keep)
        for k in c.ks:
            for r, dc in zip(c.want[k], d.cols[0]):
                xd, sd = gr.truncated(d, dc, k)[:2]
                if sd == r[1]:
                    c.drift[k] = max(c.drift[k], kr.rel_dist(xd, r[0]))
    return c


# ---- inexact sweeps (feasthip_poly_resinv_apply_dev) on damped_case("20x16", False), 16 nodes, m = 8 ----------------------------
SWEEPS = (("cocg5", "cocg", 3e-2, 50), ("cocg5", "cocg", 1e-4, 400), ("bicgstab", "bicgstab", 3e-2, 5))
SWEEP_PARAMS = [(s, shifted) for s in SWEEPS for shifted in (False, True)]
SWEEP_M = 8


def sweep_inputs():
    """(coefficients, Z, W, X, sigma): unit random columns; the shifts of the residual-inverse form are the eigenvalues inside the
    circle moved by 1e-3 (what the Ritz values of a late loop look like) and three points elsewhere in the circle."""
    case = sc.damped_case("20x16", False)
    Z, W = fo.feast_gcontour(case["center"], case["radius"], sc.NE)
    # (the seed: at (1e-4, cap 400) COCG takes up to 90 steps at the nodes next to the spectrum and 32 D of the restatement
    #  itself comes to 3e-8 .. 9e-8 over the seeds 41 .. 46; 43 leaves the largest distance to the power limit 1e-7)
    X = sc.random_block(case["N"], SWEEP_M, 43)
    X = np.asfortranarray(X / np.linalg.norm(X, axis=0))
    lam = case["lam_in"]
    sigma = np.concatenate([lam + 1e-3 * (1 + 1j), case["center"] + case["radius"] * np.array([0.3, -0.4j, 0.5 * np.exp(2.0j)])])[:SWEEP_M]
    return case["coeffs"], Z, W, X, sigma


def _sweep(op, Z, W, X, sigma, method, rtol, maxit, dots):
    ct = op.dtype
    out = np.zeros(X.shape, ct)
    cols = []
    for z, w in zip(Z, W):
        row = []
        for j in range(X.shape[1]):
            x = X[:, j].astype(ct)
            b = x if sigma is None else op.apply(sigma[j], x)
            col = kr.solve_column(op, z, b, method, rtol, 0.0, maxit, dots=dots)
            out[:, j] += ct.type(w) * col.x if sigma is None else (ct.type(w) / (ct.type(z) - ct.type(sigma[j]))) * (x - col.x)
            row.append(col)
        cols.append(row)
    return out, cols


@functools.lru_cache(maxsize=None)
def sweep_case(setting, shifted):
    method, solver, rtol, maxit = setting
    coeffs, Z, W, X, sigma = sweep_inputs()
    c = Case()
    c.coeffs, c.Z, c.W, c.X, c.sigma, c.solver, c.rtol, c.maxit = coeffs, Z, W, X, (sigma if shifted else None), solver, rtol, maxit
    N = coeffs[0].shape[0]
    c.out, cols = _sweep(PolyOp(coeffs, np.clongdouble), Z, W, X, c.sigma, method, rtol, maxit, kr.Dots(N))
    c.steps = np.array([[q.steps for q in row] for row in cols])
    c.margin = np.array([[q.margin for q in row] for row in cols])
    c.status = np.array([kr.node_status(row, rtol, 0.0) for row in cols])
    c.decided = c.margin >= MARGIN_MIN
    c.col_ok = c.decided.all(axis=0)
    ok = np.flatnonzero(c.col_ok)
    c.fp64_steps_agree, c.drift = True, 0.0
    PD = PolyOp(coeffs, np.complex128)
    for chunks, seed in kr.DRIFT_ORDERS:
        out, cols = _sweep(PD, Z, W, X, c.sigma, method, rtol, maxit, kr.Dots(N, chunks, seed))
        steps = np.array([[q.steps for q in row] for row in cols])
        c.fp64_steps_agree &= bool((steps[c.decided] == c.steps[c.decided]).all())
        c.drift = max(c.drift, kr.block_dist(out[:, ok], c.out[:, ok]))
    return c
