"""The inputs of test_gpu_krylov_steps.py and their reference results (krylov_reference.py), shared with
test_krylov_reference_host.py, which asserts on the reference alone the conditions the device comparison rests on.
Everything comes from the project's own generators with fixed seeds; reference results are cached per process."""
import functools

import numpy as np
import scipy.linalg as sla

import feast_oracle as fo
import feastkit_jl_amd as fk
import krylov_reference as kr
from ragged_cases import ragged_pair
from test_gpu_primitives import rand_block, sparse_pair

TRUNC_KS = (1, 2, 3, 5, 15, 16, 17, 31, 33, 48)
MARGIN_MIN = 1e-6          # a stop decided by less than this may fall either way on the device
LEFT_OUT_MAX = 0.02        # at most this share of the (node, column) pairs of a case may be left out for it
POWER = 1e-7               # discriminating power: 32 D of every compared case stays below this


def contour8(Emin, Emax):
    fpm = fk.feastdefault(fk.feastinit())
    fpm[2] = 8
    return fk.feast_contour(Emin, Emax, fpm)


def tile_columns(m, cap=17):
    """All columns of a narrow block; of a wide one the first and last of every 16-column tile and the last column."""
    if m <= cap:
        return list(range(m))
    s = set([m - 1])
    for t0 in range(0, m, 16):
        s.update((t0, min(t0 + 15, m - 1)))
    return sorted(s)


# ---- truncated single-shift solves ---------------------------------------------------------------------------------
def _cfg3_small():
    A, B, _ = fo.cfg3_problem(8, 7, 6)
    return A, B


def _cfg3_mid():
    A, B, _ = fo.cfg3_problem(12, 10, 9)
    return A, B


def _cfg3_big():
    A, B, _ = fk.workloads.laplacian_3d_pencil(50, 40, 30)
    return A, B


def _dense(builder):
    def f():
        A, B = builder()
        return A.toarray(), (None if B is None else B.toarray())
    return f


# BiCGStab's recurrences amplify rounding much faster than COCG's (far from the spectrum the drift of the restatement
# itself passes 1e-9 after some 25 steps, next to it after 4), so its truncated cases end at the k where the
# discriminating-power condition (32 D <= 1e-7) still holds: a smaller k, not a wider tolerance.  The host test and the
# GPU test assert the condition for every k listed here.
KS_SHORT = (1, 2, 3, 5, 15, 16, 17)
KS_NEAR = (1, 2, 3)
RAGGED_SEED = 21
# name -> (device solver, restatement, builder of (A, B), m, ks far from the spectrum, ks next to it, interval whose
#          8-node contour gives the near shift)
TRUNC = {
    "bicgstab-csr-B-N333-m17": ("bicgstab", "bicgstab", lambda: sparse_pair(333, 7), 17, KS_SHORT, KS_NEAR, (20.0, 30.0)),
    "bicgstab-csr-I-N45-m7": ("bicgstab", "bicgstab", lambda: sparse_pair(45, 8, b_identity=True), 7, TRUNC_KS, KS_NEAR, (10.0, 20.0)),
    "bicgstab-hermitian-N500-m48": ("bicgstab", "bicgstab", lambda: sparse_pair(500, 9, cplx=True), 48, KS_SHORT, KS_NEAR, (30.0, 40.0)),
    "bicgstab-dense-N203-m16": ("bicgstab", "bicgstab", _dense(lambda: sparse_pair(203, 10)), 16, TRUNC_KS, KS_NEAR, (20.0, 30.0)),
    "cocg-csr-N336-m100": ("cocg", "cocg_fused", _cfg3_small, 100, TRUNC_KS, TRUNC_KS, (0.0, 0.5)),
    "cocg-csr-N1080-m64": ("cocg", "cocg_fused", _cfg3_mid, 64, TRUNC_KS, TRUNC_KS, (0.0, 0.5)),
    "cocg-csr-N1080-m1": ("cocg", "cocg_fused", _cfg3_mid, 1, TRUNC_KS, TRUNC_KS, (0.0, 0.5)),
    "cocg-dense-N336-m7": ("cocg", "cocg5", _dense(_cfg3_small), 7, TRUNC_KS, TRUNC_KS, (0.0, 0.5)),
    "cocg-csr-N60000-m64": ("cocg", "cocg_fused", _cfg3_big, 64, (1, 2, 5), (1, 2, 5), (0.0, 0.5)),
    # ragged rows (ragged_cases.py).  m = 64 over real values: k_spmm_row and k_fused_vec; m = 17 and m = 7: k_spmm at ld 32
    # and 16, with B = I over rows without entries.  Next to the spectrum the ks are the longest prefix of the far ones that
    # keeps 32 D <= 1e-7: all of them but on N = 47, where the drift passes it at k = 31 (7e-6).  N = 47 also ends its far ks
    # at 33: COCG exhausts the Krylov space of 47 unknowns at step 47 in long double and stops there, complex128 does not
    # (fp64_steps_agree fails at k = 48): which of the two the device follows is a matter of rounding.
    "cocg-ragged-B-N323-m64": ("cocg", "cocg_fused", lambda: ragged_pair(323, RAGGED_SEED), 64, TRUNC_KS, TRUNC_KS, (0.0, 1.0)),
    "cocg-ragged-I-N331-m17": ("cocg", "cocg_fused", lambda: ragged_pair(331, RAGGED_SEED, b_identity=True), 17, TRUNC_KS, TRUNC_KS, (0.0, 12.0)),
    "cocg-ragged-I-N47-m7": ("cocg", "cocg_fused", lambda: ragged_pair(47, RAGGED_SEED, b_identity=True), 7, TRUNC_KS[:-1], KS_SHORT, (0.0, 12.0)),
    "bicgstab-ragged-B-N323-m17": ("bicgstab", "bicgstab", lambda: ragged_pair(323, RAGGED_SEED), 17, KS_SHORT, KS_NEAR, (0.0, 1.0)),
    "bicgstab-ragged-hermitian-N331-m48": ("bicgstab", "bicgstab", lambda: ragged_pair(331, RAGGED_SEED, cplx=True), 48, KS_SHORT, KS_NEAR, (0.0, 1.0)),
}
RAGGED = tuple(n for n in TRUNC if "ragged" in n)
TRUNC_HOST = ("bicgstab-csr-I-N45-m7", "bicgstab-dense-N203-m16", "cocg-csr-N1080-m1", "cocg-dense-N336-m7")
FAR_SHIFT = -3.0 + 2.0j


def near_shift(interval):
    Z, _ = contour8(*interval)
    return complex(Z[int(np.argmin(np.abs(Z.imag)))])


class TruncCase:
    pass


@functools.lru_cache(maxsize=None)
def trunc_case(name, near):
    """Reference columns run once to max(ks) with their history; per k: iterate, steps, status, margin and drift."""
    solver, method, build, m, ks_far, ks_near, interval = TRUNC[name]
    ks = ks_near if near else ks_far
    A, B = build()
    N = A.shape[0]
    c = TruncCase()
    c.solver, c.A, c.B, c.N, c.m, c.ks = solver, A, B, N, m, ks
    c.z = near_shift(interval) if near else FAR_SHIFT
    c.X = rand_block(N, m, 8)
    c.columns = tile_columns(m) if N <= 2000 else tile_columns(m)[:8]
    kmax = max(ks)
    PL = kr.Pencil(A, B, np.clongdouble)
    PD = kr.Pencil(A, B, np.complex128)
    c.ref = [kr.solve_column(PL, c.z, c.X[:, j], method, 1e-14, 0.0, kmax, keep_history=True) for j in c.columns]
    c.drift = {k: 0.0 for k in ks}
    c.fp64_steps_agree = {k: True for k in ks}        # the complex128 restatement takes the long-double one's steps up to k
    for chunks, seed in kr.DRIFT_ORDERS:
        dots = kr.Dots(N, chunks, seed)
        for j, ref in zip(c.columns, c.ref):
            d = kr.solve_column(PD, c.z, c.X[:, j], method, 1e-14, 0.0, kmax, dots=dots, keep_history=True)
            for k in ks:
                xr, sr = kr.truncated(ref, k)[:2]
                xd, sd = kr.truncated(d, k)[:2]
                c.fp64_steps_agree[k] &= sr == sd
                if sr == sd:
                    c.drift[k] = max(c.drift[k], kr.rel_dist(xd, xr))
    return c


# ---- columns that stop at different steps --------------------------------------------------------------------------
STOP_SETTINGS = ((3e-2, 0.0), (1e-3, 0.0), (1e-4, 0.0), (3e-2, 1e-6))
STOP_SOLVERS = (("cocg", "cocg_fused", False), ("cocg", "cocg5", True), ("bicgstab", "bicgstab", False))
STOP_Z = 0.33 + 0.17j


@functools.lru_cache(maxsize=None)
def stop_inputs():
    """N = 336 cfg-3 pencil; right-hand sides B v with v a sum of 1, 2, 4, ... 128 eigenvectors of the pencil under
    scales from 1e-3 to 1e3, four Gaussian columns, one column of zeros and one whose norm is below atol = 1e-6."""
    A, B, _ = fo.cfg3_problem(8, 7, 6)
    N = A.shape[0]
    _, V = sla.eigh(A.toarray(), B.toarray())
    rng = np.random.default_rng(20260515)
    cols = []
    for j in range(8):
        pick = rng.choice(N, size=2 ** j, replace=False)
        v = V[:, pick] @ rng.uniform(0.5, 1.5, size=2 ** j)
        cols.append(10.0 ** (j - 3.5) * (B @ v))
    cols += [rng.standard_normal(N) for _ in range(4)]
    cols.insert(5, np.zeros(N))
    g = rng.standard_normal(N)
    cols.insert(11, 1e-8 * g / np.linalg.norm(g))
    X = np.asfortranarray(np.array(cols).T.astype(np.complex128))
    return A, B, X


class SolveCase:
    pass


@functools.lru_cache(maxsize=None)
def stop_case(method, rtol, atol, maxit=400):
    A, B, X = stop_inputs()
    if method == "cocg5":
        A, B = A.toarray(), B.toarray()
    N, m = X.shape
    c = SolveCase()
    c.A, c.B, c.X, c.m, c.z = A, B, X, m, STOP_Z
    PL = kr.Pencil(A, B, np.clongdouble)
    PD = kr.Pencil(A, B, np.complex128)
    c.ref = [kr.solve_column(PL, c.z, X[:, j], method, rtol, atol, maxit) for j in range(m)]
    c.decided = np.array([r.margin >= MARGIN_MIN for r in c.ref])
    c.drift = np.zeros(m)
    c.fp64_steps_agree = True
    for chunks, seed in kr.DRIFT_ORDERS:
        dots = kr.Dots(N, chunks, seed)
        for j in range(m):
            d = kr.solve_column(PD, c.z, X[:, j], method, rtol, atol, maxit, dots=dots)
            if c.decided[j]:
                c.fp64_steps_agree &= d.steps == c.ref[j].steps
                c.drift[j] = max(c.drift[j], kr.rel_dist(d.x, c.ref[j].x))
    return c


# ---- inexact contour sweeps -----------------------------------------------------------------------------------------
SWEEP_SETTINGS = ((3e-2, 50), (1e-3, 60), (3e-2, 7))
SWEEP_M = (4, 24, 40, 64)
# (problem, real projection, maxit) of the BiCGStab sweeps at rtol = 3e-2.  On the Hermitian pencil BiCGStab next to the
# spectrum loses every digit to rounding within some 15 steps (drift of the restatement itself 1e-1 at maxit = 50), so that
# sweep is cut at 5 steps: three nodes stop on the tolerance after 3, the others are capped.
BICGSTAB_SWEEPS = (("cfg3", True, 50), ("cfg3", False, 50), ("hermitian", False, 5))


SWEEP_KINDS = ("cfg3", "ragged", "ragged-I")
RAGGED_SWEEP_M = (24, 64)
_SWEEP_INTERVAL = {"cfg3": (0.0, 0.5), "hermitian": (0.0, 8.0), "ragged": (0.0, 1.0), "ragged-I": (0.0, 12.0)}
_SWEEP_RITZ = {"cfg3": (0.05, 0.9), "hermitian": (-1.0, 10.0), "ragged": (-0.2, 1.5), "ragged-I": (-2.0, 15.0)}


@functools.lru_cache(maxsize=None)
def sweep_problem(kind="cfg3"):
    """(A, B, Z, W, weight scale).  cfg3: the 12 x 10 x 9 pencil and the 8-node half contour over (0, 0.5);
    hermitian: a complex Hermitian CSR pencil, N = 500, half contour over (0, 8) at the lower end of its spectrum;
    ragged: ragged_pair(323) with B, half contour over (0, 1); ragged-I: ragged_pair(331, b_identity=True), over (0, 12):
    both at the lower end, where the rows without a diagonal put their eigenvalues."""
    if kind == "cfg3":
        A, B, _ = fo.cfg3_problem(12, 10, 9)
    elif kind == "hermitian":
        A, B = sparse_pair(500, 9, cplx=True)
    elif kind == "ragged":
        A, B = ragged_pair(323, RAGGED_SEED)
    else:
        assert kind == "ragged-I", kind
        A, B = ragged_pair(331, RAGGED_SEED, b_identity=True)
    Z, W = contour8(*_SWEEP_INTERVAL[kind])
    return A, B, Z, W, 2.0


def sweep_ritz(m, kind="cfg3"):
    lo, hi = _SWEEP_RITZ[kind]                  # straddles the interval: some 1/(z_e - lambda_c) are large
    return np.linspace(lo, hi, m)


class SweepCase:
    pass


@functools.lru_cache(maxsize=None)
def sweep_case(method, rtol, maxit, m, warm, kind="cfg3", mask=False, all_columns=False):
    """Reference sweep (both projections) over the compared columns, the per-column drift of the summed block and the
    (node, column) pairs whose stop is undecidable."""
    A, B, Z, W, scale = sweep_problem(kind)
    N = A.shape[0]
    c = SweepCase()
    c.A, c.B, c.Z, c.W, c.scale, c.m = A, B, Z, W, scale, m
    c.Q = fk.seeded_subspace(N, m)
    c.ritz = sweep_ritz(m, kind) if warm else None
    c.mask = ([1, 0] * m)[:m] if mask else None
    c.columns = list(range(m)) if all_columns or m <= 24 else tile_columns(m)
    kw = dict(ritz=c.ritz, mask=c.mask, columns=c.columns)
    c.ref = kr.sweep(A, B, c.Q, Z, W, scale, False, method, rtol, 0.0, maxit, pencil=kr.Pencil(A, B, np.clongdouble), **kw)
    c.decided = c.ref.margin >= MARGIN_MIN                      # [node][compared column]
    c.col_ok = c.decided.all(axis=0)
    PD = kr.Pencil(A, B, np.complex128)
    c.fp64_steps_agree = True
    c.drift = {True: 0.0, False: 0.0}                            # by real projection
    ok = np.flatnonzero(c.col_ok)
    for chunks, seed in kr.DRIFT_ORDERS:
        d = kr.sweep(A, B, c.Q, Z, W, scale, False, method, rtol, 0.0, maxit, pencil=PD, dot_chunks=chunks, dot_seed=seed, **kw)
        c.fp64_steps_agree &= bool((d.steps[c.decided] == c.ref.steps[c.decided]).all())
        for real in (True, False):
            c.drift[real] = max(c.drift[real], kr.block_dist(project(d.out, real)[:, ok], project(c.ref.out, real)[:, ok]))
    return c


def project(out, real):
    return out.real.astype(out.dtype) if real else out
