"""The inputs of test_gpu_gmres_steps.py and their reference results (gmres_reference.py), shared with
test_gmres_reference_host.py, which asserts on the reference alone the conditions the device comparison rests on.
Everything comes from the project's own generators with fixed seeds; reference results are cached per process.
MARGIN_MIN, LEFT_OUT_MAX and POWER are those of krylov_cases.py."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feast_oracle as fo
import feastkit_jl_amd as fk
import gmres_reference as gr
import krylov_cases as kc
import krylov_reference as kr
from krylov_cases import FAR_SHIFT, LEFT_OUT_MAX, MARGIN_MIN, POWER, contour8, near_shift, project, tile_columns  # noqa: F401
from ragged_cases import ragged_pair
from test_gpu_primitives import rand_block, sparse_pair

RTOL_TRUNC = 1e-14


def nonsymmetric_pair(N=400, seed=12):
    """sparse_pair plus an unsymmetric complex part: the input class of feast_general."""
    A, B = sparse_pair(N, seed)
    U = sp.random(N, N, density=min(1.0, 3.0 / N), random_state=seed + 5, format="csr")
    L = sp.random(N, N, density=min(1.0, 3.0 / N), random_state=seed + 6, format="csr")
    return sp.csr_matrix(A + (0.7 + 0.4j) * U - 0.3j * L), B


def _dense(builder):
    def f():
        A, B = builder()
        return A.toarray(), (None if B is None else B.toarray())
    return f


def _cfg3_mid():
    A, B, _ = fo.cfg3_problem(12, 10, 9)
    return A, B


# name -> (builder of (A, B), m, restart, ks, interval whose 8-node contour gives the near shift).  With mr = max(restart, 2)
# every list of ks has a k strictly inside a cycle, one exactly on a cycle boundary and one a step after it.
TRUNC = {
    "csr-B-N333-m17-r8": (lambda: sparse_pair(333, 7), 17, 8, (1, 5, 8, 9, 16, 17, 30), (20.0, 30.0)),
    "csr-I-N45-m7-r7": (lambda: sparse_pair(45, 8, b_identity=True), 7, 7, (3, 7, 8, 14, 15, 20), (10.0, 20.0)),
    "hermitian-N500-m48-r9": (lambda: sparse_pair(500, 9, cplx=True), 48, 9, (4, 9, 10, 18, 19, 31), (30.0, 40.0)),
    "nonsym-N400-m33-r17": (nonsymmetric_pair, 33, 17, (1, 16, 17, 18, 34, 35, 40), (20.0, 30.0)),
    "dense-N203-m16-r30": (_dense(lambda: sparse_pair(203, 10)), 16, 30, (2, 29, 30, 31, 48), (20.0, 30.0)),
    "cfg3-N1080-m100-r1": (_cfg3_mid, 100, 1, (1, 2, 3, 6, 7), (0.0, 0.5)),
    "cfg3-N1080-m1-r30": (_cfg3_mid, 1, 30, (1, 15, 29, 30, 31), (0.0, 0.5)),      # (far from the spectrum it converges at 33)
    "cfg3-N1080-m24-r0": (_cfg3_mid, 24, 0, (1, 2, 3, 4), (0.0, 0.5)),
    "csr-B-N333-m17-r16": (lambda: sparse_pair(333, 7), 17, 16, (8, 15, 16, 17, 32, 33), (20.0, 30.0)),
    # ragged rows with an unsymmetric pattern (ragged_cases.py): k_spmm at ld 32 under dot mode 1 and the Arnoldi dots
    "ragged-nonsym-N323-m17-r8": (lambda: ragged_pair(323, 21, unsymmetric=True), 17, 8, (1, 5, 8, 9, 16, 17, 30), (0.0, 1.0)),
}
TRUNC_HOST = ("csr-I-N45-m7-r7", "dense-N203-m16-r30", "cfg3-N1080-m1-r30", "cfg3-N1080-m24-r0")


class Case:
    pass


def _drift_orders(N):
    return [kr.Dots(N, chunks, seed) for chunks, seed in kr.DRIFT_ORDERS]


@functools.lru_cache(maxsize=None)
def trunc_case(name, near):
    """One node, one batch: the reference run once to max(ks) with the iterates at every k kept; per k the drift."""
    build, m, restart, ks, interval = TRUNC[name]
    A, B = build()
    N = A.shape[0]
    c = Case()
    c.A, c.B, c.N, c.m, c.ks, c.restart, c.mr = A, B, N, m, ks, restart, max(restart, 2)
    c.z = near_shift(interval) if near else FAR_SHIFT
    c.X = rand_block(N, m, 8)
    c.columns = tile_columns(m)
    kmax, keep = max(ks), set(ks)
    rhs = c.X[:, c.columns]
    c.batch = gr.solve_batch(kr.Pencil(A, B, np.clongdouble), [c.z], rhs, None, RTOL_TRUNC, 0.0, kmax, restart, keep_history=keep)
    c.ref = c.batch.cols[0]
    c.want = {k: [gr.truncated(c.batch, r, k) for r in c.ref] for k in ks}       # (x, steps, status, active, margin)
    c.products = {k: gr.truncated_products(c.batch, k) for k in ks}
    c.drift = {k: 0.0 for k in ks}
    PD = kr.Pencil(A, B, np.complex128)
    for dots in _drift_orders(N):
        d = gr.solve_batch(PD, [c.z], rhs, None, RTOL_TRUNC, 0.0, kmax, restart, dots=dots, keep_history=keep)
        for k in ks:
            for r, dc in zip(c.want[k], d.cols[0]):
                xd, sd = gr.truncated(d, dc, k)[:2]
                if sd == r[1]:
                    c.drift[k] = max(c.drift[k], kr.rel_dist(xd, r[0]))
    return c


# ---- columns that stop at different steps, one node -------------------------------------------------------------------
STOP_SETTINGS = kc.STOP_SETTINGS + ((1e-10, 0.0),)
STOP_RESTARTS = (8, 30)
STOP_Z = kc.STOP_Z


@functools.lru_cache(maxsize=None)
def stop_inputs():
    """krylov_cases.stop_inputs() as a one-node sweep with weight 1: Q = B^-1 X, so that the right-hand sides B Q are the
    eigenvector sums, Gaussian columns, the zero column (5) and the column below atol = 1e-6 (11) of that block."""
    A, B, X = kc.stop_inputs()
    Q = spla.splu(sp.csc_matrix(B)).solve(X.real).astype(np.complex128)
    return A, B, np.asfortranarray(Q)


def _sweep_case(c, rtol, atol, maxit, restart, batch, ritz, columns):
    """Reference sweep in long double, the fp64 drift of the summed block (both projections), decided pairs."""
    kw = dict(batch=batch, ritz=ritz, columns=columns)
    c.ref = gr.sweep(c.A, c.B, c.Q, c.Z, c.W, c.scale, False, rtol, atol, maxit, restart,
                     pencil=kr.Pencil(c.A, c.B, np.clongdouble), **kw)
    c.decided = c.ref.margin >= MARGIN_MIN
    c.col_ok = c.decided.all(axis=0)
    c.fp64_steps_agree = True
    c.drift = {True: 0.0, False: 0.0}
    ok = np.flatnonzero(c.col_ok)
    PD = kr.Pencil(c.A, c.B, np.complex128)
    for chunks, seed in kr.DRIFT_ORDERS:
        d = gr.sweep(c.A, c.B, c.Q, c.Z, c.W, c.scale, False, rtol, atol, maxit, restart, pencil=PD, dot_chunks=chunks,
                     dot_seed=seed, **kw)
        c.fp64_steps_agree &= bool((d.steps[c.decided] == c.ref.steps[c.decided]).all())
        for real in (True, False):
            c.drift[real] = max(c.drift[real], kr.block_dist(project(d.out, real)[:, ok], project(c.ref.out, real)[:, ok]))
    return c


@functools.lru_cache(maxsize=None)
def stop_case(rtol, atol, restart, maxit=400):
    c = Case()
    c.A, c.B, c.Q = stop_inputs()
    c.Z, c.W, c.scale = np.array([STOP_Z]), np.array([1.0 + 0.0j]), 1.0
    c.m = c.Q.shape[1]
    c.columns = list(range(c.m))
    c.ritz = c.mask = None
    return _sweep_case(c, rtol, atol, maxit, restart, None, None, None)


# ---- exhaustion of the Krylov space --------------------------------------------------------------------------------------
def _tridiagonal():
    N = 12
    return sp.csr_matrix(sp.diags([-np.ones(N - 1), 2.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])), None


def _five_eigenvalues():
    d = np.repeat([1.0, 2.5, 4.0, 7.0, 11.0], 8)
    return sp.csr_matrix(sp.diags(d)), None


EXHAUST = {"tridiagonal-N12": (_tridiagonal, 12, 0.6 + 0.5j), "diagonal-5-eigenvalues": (_five_eigenvalues, 5, -0.5 + 0.7j)}


@functools.lru_cache(maxsize=None)
def exhaust_case(name):
    build, dim, z = EXHAUST[name]
    c = Case()
    c.A, c.B = build()
    N = c.A.shape[0]
    c.Q = rand_block(N, 3, 21)
    c.Z, c.W, c.scale, c.m, c.dim = np.array([z]), np.array([1.0 + 0.0j]), 1.0, 3, dim
    c.columns = [0, 1, 2]
    c.ritz = c.mask = None
    return _sweep_case(c, 1e-10, 0.0, 400, 30, None, None, None)


# ---- contour sweeps ------------------------------------------------------------------------------------------------------
SWEEP_SETTINGS = ((1e-8, 300, 20), (1e-12, 12, 10), (3e-2, 50, 30))        # (rtol, maxit, restart)
BATCHES = (8, 3, 1)
# (problem, m, Ritz warm start, setting): every m of krylov_cases.SWEEP_M, both pencils, both starts and every setting
# appear; each is run on the device with the real projection on and off under the three batch sizes.  The 300-step setting
# goes with few compared columns (the long-double reference costs a millisecond per column and step).
SWEEPS = (
    ("cfg3", 4, False, SWEEP_SETTINGS[0]),
    ("hermitian", 24, True, SWEEP_SETTINGS[2]),
    ("cfg3", 24, True, SWEEP_SETTINGS[1]),
    ("hermitian", 64, False, SWEEP_SETTINGS[1]),
    ("cfg3", 40, True, SWEEP_SETTINGS[2]),
    ("hermitian", 4, True, SWEEP_SETTINGS[0]),
    ("cfg3", 64, False, SWEEP_SETTINGS[2]),
    ("hermitian", 40, False, SWEEP_SETTINGS[0]),
)
SWEEPS_HOST = SWEEPS[:4]
MASK_SWEEP = ("cfg3", 24, True, SWEEP_SETTINGS[1])


def sweep_case(kind, m, warm, setting, batch=8):
    return _sweep_cached(kind, m, warm, tuple(setting), int(batch))


@functools.lru_cache(maxsize=None)
def _sweep_cached(kind, m, warm, setting, batch):
    """The reference under node batches of ``batch``: every batch has its own step counter, cycle starts and products."""
    rtol, maxit, restart = setting
    c = Case()
    c.A, c.B, c.Z, c.W, c.scale = kc.sweep_problem(kind)
    c.m = m
    c.Q = fk.seeded_subspace(c.A.shape[0], m)
    c.ritz = kc.sweep_ritz(m, kind) if warm else None
    c.columns = list(range(m)) if m <= 24 else tile_columns(m)
    c.mask = None
    return _sweep_case(c, rtol, 0.0, maxit, restart, batch, c.ritz, c.columns)


def budget_mb(N, m, restart, batch):
    """FH_GMRES_BUDGET_MB that makes fh_gmres take node batches of ``batch``: the basis costs (mr + 2) N ld 16 bytes per
    node and the budget is a whole number of MiB."""
    ld = 16 if m <= 16 else 32 if m <= 32 else 64
    per_node = (max(restart, 2) + 2) * N * ld * 16
    for mb in range(1, 1 << 14):
        if (mb << 20) // per_node == batch:
            return mb
    raise AssertionError("no whole-MiB budget gives batches of %d" % batch)
