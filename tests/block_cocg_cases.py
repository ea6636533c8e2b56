"""Inputs shared by test_block_cocg_reference_host.py and test_gpu_block_cocg.py: the N = 3200 Laplacian pencil, its B = I
counterpart and a variable-coefficient pencil of the same size from the project's generators; node families of 1, 3 and 8
nodes of the 16-node half contour (aspect 40) and of the circle.  Long-double restatements are cached per process; the wide
blocks run few steps (one long-double step of a 64-column block is several N x 64 x 64 products without BLAS)."""
import functools

import numpy as np
import scipy.sparse as sp

import feastkit_jl_amd as fk
import krylov_reference as kr
import block_cocg_reference as br

FAMILIES = {"1": [15], "3": [2, 15, 9], "8": [0, 2, 4, 6, 9, 11, 13, 15]}


def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


@functools.lru_cache(maxsize=None)
def problem(name):
    """(A, B or None, (Emin, Emax))"""
    if name == "lap":
        A, B, lam = fk.workloads.laplacian_3d_pencil(20, 16, 10)[:3]
        return _csr(A), _csr(B), (0.0, 0.42)
    if name == "lap-std":
        A, lam = fk.workloads.laplacian_3d_standard(20, 16, 10)[:2]
        return _csr(A), None, (0.0, 0.42)
    if name == "varcoef":
        r = fk.workloads.variable_coefficient_pencil((20, 16, 10))
        return _csr(r[0]), _csr(r[1]), (0.0, 0.5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def contour(name, aspect):
    fpm = fk.feastdefault(fk.feastinit())
    fpm[2] = 16
    if aspect != 100:
        fpm[16], fpm[18] = 0, aspect
    Z, W = fk.feast_contour(*problem(name)[2], fpm)
    return np.asarray(Z), np.asarray(W)


def ritz_guess(name, m):
    lo, hi = problem(name)[2]
    return np.linspace(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), m) + 0.0137


class Case:
    pass


# id -> (problem, family, aspect (100: the circle), m, rtol, maxit, warm, mask, duplicate column)
CASES = {
    "lap/1/m64/cap1": ("lap", "1", 40, 64, 1e-14, 1, False, False, False),
    "lap/1/m64/cap2/warm": ("lap", "1", 40, 64, 1e-14, 2, True, False, False),
    "lap/1/m63/cap2": ("lap", "1", 40, 63, 1e-14, 2, False, False, False),
    "lap/3/m17/cap7": ("lap", "3", 40, 17, 1e-14, 7, False, False, False),
    "lap/8/m5/conv": ("lap", "8", 40, 5, 3e-2, 200, False, False, False),
    "lap/8/m5/conv/warm": ("lap", "8", 40, 5, 3e-2, 200, True, False, False),
    "lap/3/m1/conv": ("lap", "3", 40, 1, 3e-2, 200, False, False, False),
    "lap-std/3/m17/conv/circle": ("lap-std", "3", 100, 17, 3e-2, 200, False, False, False),
    "varcoef/3/m17/cap7": ("varcoef", "3", 40, 17, 1e-14, 7, False, False, False),
    "lap/3/m17/mask/cap7": ("lap", "3", 40, 17, 1e-14, 7, True, True, False),
    "lap/1/m5/breakdown": ("lap", "1", 40, 5, 1e-10, 600, False, False, True),
}
CONVERGED = [k for k, v in CASES.items() if v[5] >= 200 and not v[8]]


@functools.lru_cache(maxsize=None)
def case(cid):
    name, family, aspect, m, rtol, maxit, warm, mask, dup = CASES[cid]
    A, B, _ = problem(name)
    Z, W = contour(name, aspect)
    c = Case()
    c.cid, c.A, c.B, c.m, c.rtol, c.maxit, c.scale = cid, A, B, m, rtol, maxit, 2.0
    c.Zall, c.Wall, c.nodes = Z, W, FAMILIES[family]
    c.Z, c.W = Z[c.nodes], W[c.nodes]
    c.Q = np.array(fk.seeded_subspace(A.shape[0], m))
    if dup:
        c.Q[:, 3] = c.Q[:, 1]                       # two identical right-hand sides: the start block has rank m - 1
    c.ritz = ritz_guess(name, m) if warm else None
    c.mask = ([1, 0, 1] * m)[:m] if mask else None
    kw = dict(ritz=c.ritz, mask=c.mask)
    c.ref = br.sweep(A, B, c.Q, c.Z, c.W, c.scale, False, rtol, 0.0, maxit, pencil=kr.Pencil(A, B, np.clongdouble), **kw)
    PD = kr.Pencil(A, B, np.complex128)
    c.drift, c.fp64_agree = 0.0, True
    for chunks, seed in br.DRIFT_ORDERS:
        d = br.sweep(A, B, c.Q, c.Z, c.W, c.scale, False, rtol, 0.0, maxit, pencil=PD, gram_chunks=chunks, gram_seed=seed, **kw)
        c.fp64_agree &= bool((d.steps == c.ref.steps).all() and (d.stop == c.ref.stop).all())
        c.drift = max(c.drift, kr.block_dist(d.out, c.ref.out))
    return c
