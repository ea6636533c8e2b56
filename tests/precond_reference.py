"""Restatement of the shift-preconditioned GMRES sweep (feasthip_set_preconditioner; fh_gmres with a preconditioner in
csrc/fh_api.hip, k_precond_op in csrc/fh_sparse.hip), numpy only.

The driver is gmres_reference.solve_batch, unchanged: it is handed a Pencil whose ``apply(z, x)`` is the preconditioned
operator in its identity form,

    S_e M^-1 x = x + (z_e - z_p) B M^-1 x,        M = z_p B - A,  z_p the pivot of node e,

so what it iterates is u = M x.  The device does the same: the residual b - S_e M^-1 u is the
residual b - S_e x, so targets, stop tests and step counts are those of the restatement, and the iterate is x = M^-1 u.

  arithmetic   np.clongdouble: M^-1 is a partial-pivoting LU written here (row operations confined to the band of M, which
               partial pivoting widens to kl + ku above the diagonal), applied by substitution.
               np.complex128 (the drift measurement): scipy's splu with a different ``permc_spec`` per entry of
               krylov_reference.DRIFT_ORDERS, so that the drift D contains the rounding of the factors.
  warm start   x0 = q_c / (z_e - ritz_c) becomes u0 = M x0 (one product of the plain operator at the pivot).
  finish       x = M^-1 u per column; D, and every comparison with the device, is taken on x (on the weighted sum of the x).
  products     the restatement's (one per cycle start and per lock-step) plus the product of u0 for a warm start and the
               one of the closing true residual b - S_e x: feasthip_stats.spmm_calls.
  sweeps       substitution sweeps: one per cycle start (none for the first of a zero guess), per lock-step, and the final
               x = M^-1 u: feasthip_last_precond_sweep.
All nodes of a sweep are ONE batch (the device gives every preconditioned node of a panel to one fh_gmres call).

The pivot rules (csrc/fh_precond.hpp, hip_backend.precond_plan) are restated at the end.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_reference as gr
import krylov_reference as kr

PERMC = ("COLAMD", "NATURAL", "MMD_ATA", "MMD_AT_PLUS_A")       # one per entry of kr.DRIFT_ORDERS


class BandLU:
    """P M = L U of a dense matrix in its own arithmetic, partial pivoting; rows below kl and columns beyond kl + ku of the
    diagonal are never touched (they are zero)."""

    def __init__(self, M, kl, ku):
        n = M.shape[0]
        LU = M.copy()
        self.n, self.kl, self.kv = n, kl, min(n - 1, kl + ku)
        self.piv = np.zeros(n, dtype=np.int64)
        for k in range(n):
            r1 = min(n, k + kl + 1)
            p = k + int(np.argmax(np.abs(LU[k:r1, k])))
            self.piv[k] = p
            c1 = min(n, k + self.kv + 1)
            if p != k:
                LU[[k, p], k:c1] = LU[[p, k], k:c1]
            if k + 1 < r1:
                LU[k + 1:r1, k] /= LU[k, k]
                LU[k + 1:r1, k + 1:c1] -= np.outer(LU[k + 1:r1, k], LU[k, k + 1:c1])
        self.LU = LU

    def solve(self, b):
        x = np.array(b, dtype=self.LU.dtype)
        n, LU = self.n, self.LU
        for k in range(n):
            p = self.piv[k]
            if p != k:
                x[k], x[p] = x[p], x[k]
            r1 = min(n, k + self.kl + 1)
            x[k + 1:r1] -= LU[k + 1:r1, k] * x[k]
        for k in range(n - 1, -1, -1):
            x[k] = x[k] / LU[k, k]
            r0 = max(0, k - self.kv)
            x[r0:k] -= LU[r0:k, k] * x[k]
        return x


def _bandwidths(M):
    C = sp.coo_matrix(M)
    if C.nnz == 0:
        return 0, 0
    return int(max(0, (C.row - C.col).max())), int(max(0, (C.col - C.row).max()))


class PrecondPencil(kr.Pencil):
    """apply(z, x) = x + (z - z_p) B M_p^-1 x with p = the pivot of the node whose shift is z (``zmap``: complex(z) -> pivot
    index); the plain pencil S(z) x = z B x - A x is ``plain``."""

    def __init__(self, A, B, pivots, zmap, dtype=np.clongdouble, permc_spec="COLAMD"):
        super().__init__(A, B, dtype)
        self.pivots = [complex(p) for p in pivots]
        self.zmap = dict(zmap)
        As = sp.csr_matrix(A)
        Bs = sp.identity(self.N, format="csr") if B is None else sp.csr_matrix(B)
        self.lu = []
        for zp in self.pivots:
            if self.dtype == np.complex128:
                self.lu.append(spla.splu(sp.csc_matrix(zp * Bs - As).astype(np.complex128), permc_spec=permc_spec))
            else:
                kl, ku = _bandwidths(abs(As) + abs(Bs))
                M = self.dtype.type(zp) * Bs.toarray().astype(self.dtype) - As.toarray().astype(self.dtype)
                self.lu.append(BandLU(M, kl, ku))

    def plain(self, z, x):
        return kr.Pencil.apply(self, z, x)

    def minv(self, p, x):
        return self.lu[p].solve(np.asarray(x).astype(self.dtype))

    def mul_pivot(self, p, x):
        return kr.Pencil.apply(self, self.pivots[p], x)

    def apply(self, z, x):
        p = self.zmap[complex(z)]
        c = self.dtype.type(z) - self.dtype.type(self.pivots[p])
        return x + c * self.mulB(self.minv(p, x))


class Sweep:
    """out: sum_e scale w_e x_e over the compared columns; steps / margin [node][col]; status [node]; cols: the Column
    records of the batch (their x is u; xs[node][col] is x = M^-1 u); products, sweeps, lock_steps: see the module."""
    __slots__ = ("out", "steps", "status", "margin", "cols", "xs", "products", "sweeps", "lock_steps", "batch", "pencil",
                 "warm", "W", "scale", "node_pivot")


def _weighted(P, W, scale, xs):
    ct = P.dtype
    acc = np.zeros((P.N, len(xs[0])), ct)
    for w, row in zip(W, xs):
        for j, x in enumerate(row):
            acc[:, j] += ct.type(w) * ct.type(scale) * x
    return acc


def sweep(A, B, Q, Z, W, scale, pivots, node_pivot, rtol, atol, maxit, restart, ritz=None, columns=None,
          dtype=np.clongdouble, dot_chunks=0, dot_seed=0, permc_spec="COLAMD", keep=None):
    """The image of feasthip_contour_apply with solver GMRES under feasthip_set_preconditioner(pivots, node_pivot): every
    node preconditioned, zero guess or the Ritz warm start.  ``keep``: the lock-step counts k for which truncated() is wanted."""
    zmap = {complex(z): int(p) for z, p in zip(Z, node_pivot)}
    P = PrecondPencil(A, B, pivots, zmap, dtype, permc_spec)
    ct = P.dtype
    columns = list(range(Q.shape[1])) if columns is None else list(columns)
    Qc = np.asarray(Q)[:, columns].astype(ct)
    rhs = np.stack([P.mulB(Qc[:, j]) for j in range(len(columns))], axis=1)
    u0s = None
    if ritz is not None:
        lam = np.asarray(ritz)[columns].astype(P.real)
        u0s = []
        for z, p in zip(Z, node_pivot):
            x0 = Qc / (ct.type(z) - lam.astype(ct))[None, :]
            u0s.append(np.stack([P.mul_pivot(p, x0[:, j]) for j in range(len(columns))], axis=1))
    b = gr.solve_batch(P, list(Z), rhs, u0s, rtol, atol, maxit, restart, dots=kr.Dots(P.N, dot_chunks, dot_seed),
                       keep_history=set(keep) if keep else False)
    res = Sweep()
    res.batch, res.pencil, res.cols, res.warm, res.W, res.scale, res.node_pivot = b, P, b.cols, ritz is not None, W, scale, list(node_pivot)
    res.xs = [[P.minv(p, c.x) for c in row] for p, row in zip(node_pivot, b.cols)]
    res.out = _weighted(P, W, scale, res.xs)
    res.steps = np.array([[c.steps for c in row] for row in b.cols], dtype=np.int64)
    res.margin = np.array([[c.margin for c in row] for row in b.cols])
    res.status = np.array([gr.node_status(row) for row in b.cols], dtype=np.int64)
    res.lock_steps = b.lock_steps
    res.products = b.products + 1 + (1 if res.warm else 0)
    res.sweeps = b.cycles - (0 if res.warm else 1) + b.lock_steps + 1
    return res


def truncated(res, k):
    """The sweep cut at maxit = k (k in ``keep``): (out, steps, status, margin, products, sweeps)."""
    b, P = res.batch, res.pencil
    cut = [[gr.truncated(b, c, k) for c in row] for row in b.cols]           # (u, steps, status, active, margin)
    xs = [[P.minv(p, t[0]) for t in row] for p, row in zip(res.node_pivot, cut)]
    steps = np.array([[t[1] for t in row] for row in cut], dtype=np.int64)
    margin = np.array([[t[4] for t in row] for row in cut])
    status = np.array([kr.NO_CONVERGENCE if any(t[3] for t in row) else 0 for row in cut], dtype=np.int64)
    ran = min(k, b.lock_steps)
    starts = gr.truncated_products(b, k) - ran
    extra = 1 + (1 if res.warm else 0)
    return _weighted(P, res.W, res.scale, xs), steps, status, margin, gr.truncated_products(b, k) + extra, starts - (0 if res.warm else 1) + ran + 1


# ---- the pivot rules ------------------------------------------------------------------------------------------------------
def arc_pivots(ne, k):
    """csrc/fh_precond.hpp: arc a = nodes [a ne // k, (a + 1) ne // k), its pivot the middle node (of two, the lower one in
    the first half of the arcs and the upper one in the second)."""
    k = max(1, min(int(k), ne))
    node_pivot, pivot_node = [-1] * ne, []
    for a in range(k):
        lo, hi = a * ne // k, (a + 1) * ne // k
        pivot_node.append(lo + (hi - lo - 1) // 2 if 2 * a + 1 <= k else lo + (hi - lo) // 2)
        node_pivot[lo:hi] = [a] * (hi - lo)
    return node_pivot, pivot_node


def nearest_pivots(Z, pivots):
    return [int(np.argmin([abs(complex(z) - complex(p)) ** 2 for p in pivots])) for z in Z]
