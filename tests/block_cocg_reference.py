"""Restatement of the block COCG sweep (csrc/fh_api.hip: fh_block_cocg; csrc/fh_bcocg.hip: k_bcocg_gram, k_bcocg_small,
k_bcocg_update), numpy only, step for step.

Per node the live columns (unmasked, non-zero start residual above its target) form one block.  With the shared start
R0 = src diag(f) (src = B q, f = 1 from a zero guess; src = A q - ritz B q, f = 1 / (z - ritz) from the Ritz warm start):

    start   SH = src^H src, ST = src^T src;  H = E D_f^H SH D_f E^T (live columns);  zeta0 = equilibrated Cholesky factor of H
            C[:, live] = zeta0;  Zi = E^T D_f zeta0^-1;  Q = P = src Zi;  T = Zi^T ST Zi
    step    W = S P;  G = P^T W;  alpha = G^-1 T (LU, partial pivoting);  X += P (alpha C);  Qh = Q - W alpha
            GH = Qh^H Qh, GT = Qh^T Qh;  zeta from GH;  U = GT zeta^-1;  T' = zeta^-T U;  beta = T^-1 U (LU);  T = T'
            C <- zeta C;  |r_c| = |C e_c|_2;  the node stops when every live column is at or below its target
            Q = Qh zeta^-1;  P = Q + P beta
    breakdown (the node leaves with the X it has): the Cholesky meets a pivot of the equilibrated matrix <= 1e-10 or a
            non-positive diagonal; an LU pivot below 1e-13 times the largest entry; anything not finite.  The per-column COCG
            (krylov_reference.solve_column, "cocg_fused") then solves S d = (panel that Q holds) C column by column.

The arithmetic type is a parameter (np.clongdouble: the reference; np.complex128 with permuted, chunked Gram sums: the drift
measurement), as in krylov_reference.py.
"""
import numpy as np

import krylov_reference as kr

CHOL_TOL = 1e-10
PIVOT_TOL = 1e-13
RUNNING, CONVERGED, BREAKDOWN = 0, 1, 2


class Grams:
    """X^H Y or X^T Y.  chunks == 0: one product; chunks > 0: rows permuted (seeded), split into interleaved sets, each set's
    product on its own, the partial products added in order (the device sums per-workgroup partial tiles)."""

    def __init__(self, N, chunks=0, seed=0):
        self.chunks = int(chunks)
        self.perm = np.random.default_rng([seed, N, self.chunks]).permutation(N) if self.chunks else None

    def __call__(self, X, Y, conj):
        Xt = (np.conj(X) if conj else X).T
        if not self.chunks:
            return Xt @ Y
        tot = np.zeros((X.shape[1], Y.shape[1]), X.dtype)
        for j in range(self.chunks):
            rows = self.perm[j::self.chunks]
            tot = tot + Xt[:, rows] @ Y[rows]
        return tot


def _finite(M):
    return bool(np.isfinite(M.real).all() and np.isfinite(M.imag).all())


def chol_zeta(H):
    """(zeta, zeta^-1) with H = zeta^H zeta from the equilibrated Cholesky, or None when the block has lost rank."""
    n = H.shape[0]
    ct = H.dtype
    g = H.diagonal().real
    if not (np.isfinite(g).all() and (g > 0).all()) or not _finite(H):
        return None
    d = np.sqrt(g)
    A = H / np.outer(d, d)
    for k in range(n):
        pv = A[k, k].real
        if not (pv > CHOL_TOL) or not np.isfinite(pv):
            return None
        r = np.sqrt(pv)
        A[k + 1:, k] = A[k + 1:, k] * (1 / r)
        A[k, k] = r
        if k + 1 < n:
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(A[k + 1:, k], np.conj(A[k + 1:, k]))
    L = np.tril(A)
    zeta = (np.conj(L).T * d[None, :]).astype(ct)
    Zi = np.eye(n, dtype=ct)
    for k in range(n - 1, -1, -1):
        Zi[k] = Zi[k] * (1 / zeta[k, k].real)
        if k:
            Zi[:k] = Zi[:k] - np.outer(zeta[:k, k], Zi[k])
    return zeta, Zi


def lu_solve(A, B):
    """A^-1 B by LU with partial pivoting (ties: the lowest row), or None on a small or non-finite pivot."""
    A = A.copy(); B = B.copy()
    n = A.shape[0]
    if not (_finite(A) and _finite(B)):
        return None
    amax = np.sqrt((A.real ** 2 + A.imag ** 2).max())
    for k in range(n):
        v = A[k:, k].real ** 2 + A[k:, k].imag ** 2
        p = k + int(np.argmax(v))
        vm = v[p - k]
        if not (np.sqrt(vm) >= PIVOT_TOL * amax) or not (vm > 0) or not np.isfinite(vm):
            return None
        if p != k:
            A[[k, p]] = A[[p, k]]; B[[k, p]] = B[[p, k]]
        if k + 1 < n:
            l = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(l, A[k, k + 1:])
            B[k + 1:] = B[k + 1:] - np.outer(l, B[k])
    for k in range(n - 1, -1, -1):
        B[k] = B[k] / A[k, k]
        if k:
            B[:k] = B[:k] - np.outer(A[:k, k], B[k])
    return B


class Node:
    """What one node did.  X: its solution update (N x m, unweighted, without the warm start); steps, passes; stop (1 converged,
    2 breakdown, 0 capped); live: the block's columns; rnorm, target, r0norm, active per column; Rrec: the recurrence residual
    panel (N x m: the panel Q holds times C); fallback: per-column records of the finishing sweep (breakdown only)."""


def node_solve(P, z, src, f, rtol, atol, maxit, mask=None, grams=None, fallback_maxit=None):
    ct, rt = P.dtype, P.real
    N, m = src.shape
    grams = grams or Grams(N)
    z = ct.type(z)
    src = src.astype(ct); f = np.asarray(f).astype(ct)
    out = Node()
    SH, ST = grams(src, src, True), grams(src, src, False)
    g = SH.diagonal().real
    d = np.abs(f) * np.sqrt(np.where(g > 0, g, 0))
    target = rt.type(rtol) * d + rt.type(atol)
    on = np.isfinite(d) & (d > target)
    if mask is not None:
        on &= np.asarray(mask[:m], dtype=bool)
    live = np.flatnonzero(on)
    n = len(live)
    out.live, out.r0norm, out.target = live, d.astype(float), target.astype(float)
    out.rnorm = d.astype(float).copy()
    out.active = on.copy()
    out.iters = np.zeros(m, dtype=np.int64)
    out.steps = out.passes = 0
    out.X = np.zeros((N, m), ct)
    out.fallback = None
    out.Rrec = src * f[None, :] * on[None, :]
    if n == 0:
        out.stop = CONVERGED
        return out
    out.stop = RUNNING
    H = np.conj(f[live])[:, None] * SH[np.ix_(live, live)] * f[live][None, :]
    cz = chol_zeta(H)
    Qpanel, C = None, None
    if cz is None:
        out.stop = BREAKDOWN
    else:
        zeta0, Zi0 = cz
        C = np.zeros((n, m), ct); C[:, live] = zeta0
        Zi = np.zeros((m, n), ct); Zi[live] = f[live][:, None] * Zi0
        T = Zi.T @ (ST @ Zi)
        Q = src @ Zi
        Pn = Q.copy()
        Qpanel = Q
    while out.stop == RUNNING and out.steps < maxit:
        W = np.stack([P.apply(z, Pn[:, j]) for j in range(n)], axis=1)
        out.passes += 1
        G = grams(Pn, W, False)
        al = lu_solve(G, T)
        if al is None:
            out.stop = BREAKDOWN; break
        out.steps += 1
        out.X += Pn @ (al @ C)
        Qh = Q - W @ al
        Qpanel = Qh
        cz = chol_zeta(grams(Qh, Qh, True))
        if cz is None:
            out.stop = BREAKDOWN; break
        zeta, Zi = cz
        U = grams(Qh, Qh, False) @ Zi
        Tn = Zi.T @ U
        be = lu_solve(T, U)
        if be is None:
            out.stop = BREAKDOWN; break
        T = Tn
        C = zeta @ C
        rn = np.sqrt((C.real ** 2 + C.imag ** 2).sum(axis=0))
        out.rnorm[live] = rn[live].astype(float)
        out.iters[live] = out.steps
        out.active[live] = ~(rn[live] <= target[live])
        if not np.isfinite(rn[live]).all():
            out.stop = BREAKDOWN; break
        Q = Qh @ Zi
        Qpanel = Q
        if not out.active[live].any():
            out.stop = CONVERGED; break
        Pn = Q + Pn @ be
    if Qpanel is not None:
        out.Rrec = Qpanel @ C
    if out.stop == BREAKDOWN:
        out.fallback = []
        for c in range(m):
            col = kr.solve_column(P, z, out.Rrec[:, c], "cocg_fused", rtol, atol, fallback_maxit or maxit,
                                  masked=bool(mask is not None and not mask[c]))
            out.X[:, c] += col.x
            out.fallback.append(col)
            out.iters[c] += col.steps
        out.passes += max(c.steps for c in out.fallback)
    return out


def node_status(nd, rtol, atol):
    """fh_collect_columns on the block sweep's per-column words, or on the finishing sweep's after a breakdown."""
    if nd.fallback is not None:
        return kr.node_status(nd.fallback, rtol, atol)
    return kr.NO_CONVERGENCE if (nd.active.any() or not np.isfinite(nd.rnorm).all()) else 0


class Sweep:
    __slots__ = ("out", "nodes", "steps", "stop", "passes", "status", "steps_max", "breakdowns")


def sweep(A, B, Q, Z, W, scale, real_part, rtol, atol, maxit, ritz=None, mask=None, dtype=np.clongdouble, gram_chunks=0,
          gram_seed=0, pencil=None):
    """The image of feasthip_contour_apply under solver "block_cocg": out = [Re] sum_e scale w_e Y_e."""
    P = pencil or kr.Pencil(A, B, dtype)
    ct = P.dtype
    N, m = Q.shape
    grams = Grams(N, gram_chunks, gram_seed)
    Qc = np.asarray(Q).astype(ct)
    BQ = np.stack([P.mulB(Qc[:, c]) for c in range(m)], axis=1)
    if ritz is None:
        src = BQ
    else:
        src = np.stack([P.mulA(Qc[:, c]) for c in range(m)], axis=1) - BQ * np.asarray(ritz).astype(P.real)[None, :]
    res = Sweep()
    res.nodes = []
    acc = np.zeros((N, m), ct)
    for z, w in zip(Z, W):
        f = np.ones(m, ct) if ritz is None else 1 / (ct.type(z) - np.asarray(ritz).astype(ct))
        nd = node_solve(P, z, src, f, rtol, atol, maxit, mask=mask, grams=grams)
        ws = ct.type(w) * ct.type(scale)
        acc += ws * nd.X
        if ritz is not None:
            acc += ws * Qc * f[None, :]
        res.nodes.append(nd)
    res.out = acc.real.astype(ct) if real_part else acc
    res.steps = np.array([nd.steps for nd in res.nodes])
    res.stop = np.array([nd.stop for nd in res.nodes])
    res.passes = int(sum(nd.passes for nd in res.nodes))
    res.status = np.array([node_status(nd, rtol, atol) for nd in res.nodes])
    res.steps_max = int(res.steps.max())
    res.breakdowns = int((res.stop == BREAKDOWN).sum())
    return res


DRIFT_ORDERS = ((0, 0), (7, 1), (32, 2))       # (interleaved chunks, permutation seed) of the three fp64 runs


def tolerance(D):
    """The device result must lie within max(32 D, 64 eps) of the long-double restatement (D: its own complex128 drift over
    DRIFT_ORDERS), as krylov_reference.tolerance."""
    return kr.tolerance(D)
