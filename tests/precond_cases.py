"""The inputs of test_gpu_precond.py and their reference results (precond_reference.py), shared with
test_precond_reference_host.py, which asserts on the reference alone the conditions the device comparison rests on.
Everything comes from the project's own generators with fixed seeds; reference results are cached per process.
MARGIN_MIN, LEFT_OUT_MAX and POWER are those of krylov_cases.py.

Every case is an 8-node half-contour sweep (krylov_cases.contour8) from a zero guess (one from the Ritz warm start) with
rtol = 1e-10: all eight nodes in one batch, every node preconditioned.  Pivots: an explicit shift off the contour, or
"arcs:k" -- the rule of precond_shifts=k (k arcs of the nodes in order, each arc's middle node).  The random pencils have a
spectrum that is dense inside the interval, where restarted GMRES stalls under ONE pivot whatever the restart length
(test_precond_reference_host.py shows it); their pinned cases take two.
"""
import functools

import numpy as np
import scipy.sparse as sp

import feast_oracle as fo
import feastkit_jl_amd as fk
import krylov_reference as kr
import precond_reference as pr
from gmres_cases import nonsymmetric_pair
from krylov_cases import LEFT_OUT_MAX, MARGIN_MIN, POWER, contour8, project, tile_columns  # noqa: F401
from ragged_cases import ragged_pair
from test_gpu_primitives import sparse_pair

RTOL = 1e-10
MAXIT = 200


def _cfg3_small():
    A, B, _ = fo.cfg3_problem(8, 7, 6)
    return A, B


def _cfg3_mid():
    A, B, _ = fo.cfg3_problem(12, 10, 9)
    return A, B


def _tridiagonal():
    """1-D Laplacian, B = I: kl + ku = 2, the narrow band plan of the direct solver; ten eigenvalues inside (0, 0.05)."""
    N = 150
    return sp.csr_matrix(sp.diags([-np.ones(N - 1), 2.0 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1])), None


TOP = (0.25 + 0.25j,)          # the top of the circle over (0, 0.5): no node of the 8-node contour
# name -> (builder of (A, B), m, interval, pivots, restart, warm start, truncation ks)
CASES = {
    "cfg3-N336-m16-r10": (_cfg3_small, 16, (0.0, 0.5), TOP, 10, False, (1, 10, 11)),
    "cfg3-N1080-m5-r20": (_cfg3_mid, 5, (0.0, 0.5), TOP, 20, False, ()),
    "csr-B-N333-m5-r30": (lambda: sparse_pair(333, 7), 5, (20.0, 30.0), "arcs:2", 30, False, ()),
    "nonsym-N400-m5-r30": (nonsymmetric_pair, 5, (20.0, 30.0), "arcs:2", 30, False, ()),
    "csr-I-N45-m7-r30": (lambda: sparse_pair(45, 8, b_identity=True), 7, (10.0, 20.0), "arcs:2", 30, False, ()),
    "ragged-nonsym-N323-m17-r8": (lambda: ragged_pair(323, 21, unsymmetric=True), 17, (0.0, 1.0), "arcs:2", 8, False, (1, 8, 9)),
    "cfg3-N336-m64-r10": (_cfg3_small, 64, (0.0, 0.5), TOP, 10, False, ()),
    "cfg3-N336-m100-r10": (_cfg3_small, 100, (0.0, 0.5), TOP, 10, False, ()),
    "cfg3-N336-m16-r10-warm": (_cfg3_small, 16, (0.0, 0.5), TOP, 10, True, ()),
    "tridiag-I-N150-m3-r30": (_tridiagonal, 3, (0.0, 0.05), "arcs:2", 30, False, ()),
}


class Case:
    pass


def pivots_of(spec, Z):
    """(pivot shifts, node -> pivot)"""
    if isinstance(spec, str):
        node_pivot, pivot_node = pr.arc_pivots(len(Z), int(spec.split(":")[1]))
        return [complex(Z[e]) for e in pivot_node], node_pivot
    piv = [complex(p) for p in spec]
    return piv, pr.nearest_pivots(Z, piv)


@functools.lru_cache(maxsize=None)
def case(name):
    build, m, interval, spec, restart, warm, ks = CASES[name]
    c = Case()
    c.name, c.m, c.restart, c.mr, c.ks = name, m, restart, max(restart, 2), ks
    c.A, c.B = build()
    c.N = c.A.shape[0]
    c.Z, c.W = contour8(*interval)
    c.scale = 2.0
    c.pivots, c.node_pivot = pivots_of(spec, c.Z)
    c.Q = fk.seeded_subspace(c.N, m)
    c.ritz = np.linspace(interval[0] - 0.2 * (interval[1] - interval[0]), interval[1] + 0.2 * (interval[1] - interval[0]), m) if warm else None
    c.columns = list(range(m)) if m <= 24 else tile_columns(m)
    args = (c.A, c.B, c.Q, c.Z, c.W, c.scale, c.pivots, c.node_pivot, RTOL, 0.0, MAXIT, restart)
    kw = dict(ritz=c.ritz, columns=c.columns, keep=ks)
    c.ref = pr.sweep(*args, **kw)
    c.decided = c.ref.margin >= MARGIN_MIN
    c.col_ok = c.decided.all(axis=0)
    c.trunc = {k: pr.truncated(c.ref, k) for k in ks}          # (out, steps, status, margin, products, sweeps)
    c.drift = {True: 0.0, False: 0.0}
    c.trunc_drift = {k: 0.0 for k in ks}
    c.fp64_steps_agree = True
    c.node_drift = [0.0] * len(c.Z)            # of one node's own block of x (feasthip_shifted_solve)
    ok = np.flatnonzero(c.col_ok)
    for (chunks, seed), permc in zip(kr.DRIFT_ORDERS, pr.PERMC):
        d = pr.sweep(*args, dtype=np.complex128, dot_chunks=chunks, dot_seed=seed, permc_spec=permc, **kw)
        c.fp64_steps_agree &= bool((d.steps[c.decided] == c.ref.steps[c.decided]).all())
        for real in (True, False):
            c.drift[real] = max(c.drift[real], kr.block_dist(project(d.out, real)[:, ok], project(c.ref.out, real)[:, ok]))
        for e in range(len(c.Z)):
            c.node_drift[e] = max(c.node_drift[e], kr.block_dist(np.stack(d.xs[e], axis=1), np.stack(c.ref.xs[e], axis=1)))
        for k in ks:
            t, r = pr.truncated(d, k), c.trunc[k]
            good = np.flatnonzero(((r[3] >= MARGIN_MIN) & (t[1] == r[1])).all(axis=0))
            c.trunc_drift[k] = max(c.trunc_drift[k], kr.block_dist(t[0][:, good], r[0][:, good]))
    return c
