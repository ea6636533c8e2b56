"""Inputs shared by test_shifted_reference_host.py and test_gpu_shifted_cocg.py: standard problems (B = None, real
symmetric CSR A) from the project's own generators, the 16-node half contour, node families of 1, 3 and 16 nodes.
Reference results are cached per process."""
import functools

import numpy as np

import feast_oracle as fo
import feastkit_jl_amd as fk
import krylov_reference as kr
import shifted_krylov_reference as skr
import scipy.sparse as sp
from ragged_cases import ragged_pair

MARGIN_MIN = 1e-6
POWER = 1e-7
TRUNC_KS = (1, 2, 3, 5, 16, 17, 33)
INEXACT = ((3e-2, 60), (1e-3, 80))
FAMILIES = {"1": [7], "3": [2, 15, 9], "16": list(range(16))}

def _rand_csr(N, seed):
    """Random symmetric CSR matrix with the diagonal 1 .. N (the B = None case of krylov_cases.py: sparse_pair(45, 8,
    b_identity=True) of test_gpu_primitives.py, restated here so that the host test imports no GPU test module)."""
    A = sp.random(N, N, density=min(1.0, 6.0 / N), random_state=seed, format="csr")
    return sp.csr_matrix(A + A.T + sp.diags(np.arange(1, N + 1, dtype=float)))


# name -> (builder of A, interval of the 16-node contour, Ritz guesses straddle it)
PROBLEMS = {
    "lap-N336": (lambda: fo.cfg3_problem(8, 7, 6)[0], (0.4, 1.5)),
    "lap-N1080": (lambda: fo.cfg3_problem(12, 10, 9)[0], (0.2, 0.9)),
    "rand-N45": (lambda: _rand_csr(45, 8), (10.0, 20.0)),
    # ragged rows, some without entries (ragged_cases.py); the interval at the low end of the spectrum, where the rows
    # without a diagonal put their eigenvalues
    "ragged-I-N331": (lambda: ragged_pair(331, 21, b_identity=True)[0], (0.0, 12.0)),
}
RAGGED = "ragged-I-N331"
HOST_M = 3          # columns the host test compares
LD_M = {16: 9, 32: 24, 64: 40}


def contour16(Emin, Emax):
    fpm = fk.feastdefault(fk.feastinit())
    fpm[2] = 16
    return fk.feast_contour(Emin, Emax, fpm)


@functools.lru_cache(maxsize=None)
def problem(name):
    build, interval = PROBLEMS[name]
    A = build().tocsr()
    A.sort_indices()
    Z, W = contour16(*interval)
    return A, np.asarray(Z), np.asarray(W), interval


def ritz_guess(name, m):
    lo, hi = PROBLEMS[name][1]
    return np.linspace(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), m) + 0.0137      # (never an eigenvalue of these matrices)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def sweep_case(name, family, rtol, maxit, m, warm, mask=False, plain_weights=False):
    """Long-double shifted restatement of one sweep, its fp64 drift over kr.DRIFT_ORDERS and the decidable pairs.
    plain_weights: every node weighs 1 (scale 1) instead of its quadrature weight -- the sum over the nodes then does not
    cancel the way the contour filter does on a vector outside the interval."""
    A, Z, W, _ = problem(name)
    if plain_weights:
        W = np.ones_like(W)
    nodes = FAMILIES[family]
    c = Case()
    c.A, c.Z, c.W, c.nodes, c.m, c.scale = A, Z[nodes], W[nodes], nodes, m, (1.0 if plain_weights else 2.0)
    c.Zall, c.Wall = Z, W
    c.Q = fk.seeded_subspace(A.shape[0], m)
    c.ritz = ritz_guess(name, m) if warm else None
    c.mask = ([1, 0, 1] * m)[:m] if mask else None
    c.columns = list(range(m)) if m <= 12 else sorted(set([0, 1, m // 2, m - 2, m - 1] + list(range(15, m, 16)) + list(range(16, m, 16))))
    kw = dict(ritz=c.ritz, mask=c.mask, columns=c.columns)
    c.ref, c.seed, c.passes = skr.sweep(A, c.Q, c.Z, c.W, c.scale, rtol, 0.0, maxit, pencil=kr.Pencil(A, None, np.clongdouble), **kw)
    c.decided = c.ref.margin >= MARGIN_MIN
    c.col_ok = c.decided.all(axis=0)
    PD = kr.Pencil(A, None, np.complex128)
    ok = np.flatnonzero(c.col_ok)
    c.drift = {True: 0.0, False: 0.0}
    c.fp64_steps_agree = True
    for chunks, seed in kr.DRIFT_ORDERS:
        d, _, _ = skr.sweep(A, c.Q, c.Z, c.W, c.scale, rtol, 0.0, maxit, pencil=PD, dot_chunks=chunks, dot_seed=seed, **kw)
        c.fp64_steps_agree &= bool((d.steps[c.decided] == c.ref.steps[c.decided]).all())
        for real in (True, False):
            pr = (lambda o: o.real.astype(o.dtype)) if real else (lambda o: o)
            c.drift[real] = max(c.drift[real], kr.block_dist(pr(d.out)[:, ok], pr(c.ref.out)[:, ok]))
    return c
