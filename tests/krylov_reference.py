"""Per-column restatement of the batched Krylov solvers of csrc/fh_api.hip (fh_krylov) and csrc/fh_sparse.hip
(k_fin_init, k_fin_alpha, k_fin_omega, k_fin_rho, k_fused_fin, k_fused_vec, k_xr_update, k_cocg_update), numpy only.

One column and one shift at a time; the arithmetic type is a parameter (np.clongdouble: the reference proper,
np.complex128: the drift measurement) and the dots may be summed over permuted rows in interleaved chunks (again only for
the drift measurement).  The recurrences, the order of the tests inside a step and every stop rule are those of the
kernels, not of a textbook:

  bicgstab    method 0.  rhat = r0, rho = |r0|^2; sigma = <rhat, v> = sum conj(rhat) v (k_spmm dot_mode 1: cmulc(U, y)),
              alpha = rho / sigma; s = r - alpha v; <t, s> = sum conj(t) s (dot_mode 2: cmulc(y, x)), omega = <t,s>/<t,t>
              (0 when <t,t> == 0); x += alpha p + omega s; r = s - omega t; rho' = sum conj(rhat) r (k_xr_update); the stop
              test after the whole step (k_fin_rho); beta = (rho'/rho)(alpha/omega); p = r + beta (p - omega v).
  cocg5       method 1, five launches (FH_COCG_FUSED=0, and always for a dense operator): sigma = p^T S p, alpha = rho/sigma,
              x += alpha p, r -= alpha q, rho' = r^T r (unconjugated), stop test, beta = rho'/rho, p = r + beta p.
  cocg_fused  method 1 over a CSR operator (k_fused_fin): the stop test on the TRUE norm of the residual runs at the head of
              the next iteration (one product late) or in the final check after the last queued step; alpha = rho/sigma with
              the true rho; rho' = alpha^2 kappa - rho (kappa = q^T q), beta = rho'/rho; with rtol >= 1e-3 and atol == 0 a
              column whose |rho'| (|r|^2/|r^T r|) is <= target^2 (and >= 1e-12 |r|^2) takes this step and stops: beta = 0,
              the reported norm is the square root of the estimate.

Common (k_fin_init, fh_collect_columns at the end of fh_krylov): target = rtol |r0| + atol; a column with |r0| <= target, a masked
column or a non-finite |r0| never iterates; breakdown (sigma == 0, rho == 0, non-finite alpha / beta) ends the column with
status 8; maxit caps the steps; a node reports 5 when a column is still active, its norm is not finite, or it broke down
above its target.
"""
import numpy as np

NO_CONVERGENCE = 5
BREAKDOWN = 8
METHODS = ("bicgstab", "cocg5", "cocg_fused")


class Pencil:
    """S(z) x = z B x - A x in the arithmetic of ``dtype``.  A, B: dense arrays or scipy sparse matrices (B None: identity).
    Sparse products are row sums over the CSR arrays (every type numpy has, long double included); a row without entries
    gives zero."""

    def __init__(self, A, B=None, dtype=np.clongdouble):
        self.dtype = np.dtype(dtype)
        self.real = np.zeros(1, self.dtype).real.dtype
        self.N = A.shape[0]
        self.A = self._prep(A)
        self.B = None if B is None else self._prep(B)

    def _prep(self, M):
        if hasattr(M, "tocsr"):
            M = M.tocsr()
            M.sort_indices()
            cplx = np.iscomplexobj(M.data)
            data = M.data.astype(self.dtype if cplx else self.real)
            if self.dtype == np.complex128:
                return ("scipy", M.astype(np.complex128 if cplx else np.float64))
            filled = np.diff(M.indptr) > 0
            # a row without entries gives zero: reduceat sums from each listed start to the next, so it gets the starts of the
            # rows that have entries and the others keep the zero (rows = None: every row has one, the sums are the result)
            return ("csr", data, M.indices.copy(), M.indptr[:-1][filled].copy(), None if filled.all() else np.flatnonzero(filled))
        M = np.asarray(M)
        return ("dense", M.astype(self.dtype if np.iscomplexobj(M) else self.real))

    def _mul(self, M, x):
        if M[0] == "scipy":
            return M[1] @ x
        if M[0] == "dense":
            return M[1] @ x
        _, data, idx, ptr, rows = M
        if rows is None:
            return np.add.reduceat(data * x[idx], ptr)
        y = np.zeros(self.N, dtype=np.result_type(data, x))
        if len(ptr):
            y[rows] = np.add.reduceat(data * x[idx], ptr)
        return y

    def mulA(self, x):
        return self._mul(self.A, x)

    def mulB(self, x):
        return x.copy() if self.B is None else self._mul(self.B, x)

    def apply(self, z, x):
        return self.dtype.type(z) * self.mulB(x) - self.mulA(x)


class Dots:
    """sum u*v (conj=False) or sum conj(u)*v (conj=True).  chunks == 0: numpy's own order; chunks > 0: rows permuted
    (seeded), split into ``chunks`` interleaved sets, each summed on its own, then the partial sums added in order."""

    def __init__(self, N, chunks=0, seed=0):
        self.chunks = int(chunks)
        self.perm = np.random.default_rng([seed, N, self.chunks]).permutation(N) if self.chunks else None

    def __call__(self, u, v, conj=False):
        w = (np.conj(u) if conj else u) * v
        if not self.chunks:
            return w.sum()
        w = w[self.perm]
        n = (len(w) // self.chunks) * self.chunks
        part = w[:n].reshape(-1, self.chunks).sum(axis=0)         # chunk j: rows j, j + chunks, ... in order
        part[:len(w) - n] += w[n:]
        tot = w.dtype.type(0)
        for v in part:
            tot = tot + v
        return tot


class Column:
    """What one column did.  x: the iterate it ended with; steps: k_fin_rho / k_fused_fin's ``iters``; status 0 or 8;
    active: still iterating when maxit was reached; rnorm: the reported norm; margin: the smallest |lhs/rhs - 1| over the
    stop comparisons evaluated.  history (when asked for): after step k, history[k] = (x_k, rnorm_k, margin_k) with the
    comparisons up to and including the norm test that follows step k; history[0] is the start."""
    __slots__ = ("x", "steps", "status", "active", "rnorm", "r0norm", "target", "margin", "history")


def _finite(v):
    return bool(np.isfinite(v.real) and np.isfinite(v.imag))


def _margin(lhs, rhs):
    lhs, rhs = float(lhs), float(rhs)
    if not (np.isfinite(lhs) and np.isfinite(rhs)):
        return np.inf
    if rhs == 0.0:
        return np.inf          # a zero threshold (zero column: 0 > 0 is false in every arithmetic) is not a matter of rounding
    return abs(lhs / rhs - 1.0)


def solve_column(pencil, z, b, method, rtol, atol, maxit, x0=None, masked=False, dots=None, keep_history=False):
    assert method in METHODS
    ct = pencil.dtype
    rt = pencil.real
    dots = dots or Dots(pencil.N)
    z = ct.type(z)
    b = np.asarray(b).astype(ct)
    x = np.zeros(pencil.N, ct) if x0 is None else np.asarray(x0).astype(ct)
    out = Column()
    # R = RHS - S X0, |R|^2 (dot_mode 3); k_fin_init
    r = b - pencil.apply(z, x)
    rr = dots(r, r, conj=True).real
    rn = np.sqrt(rr)
    target = rt.type(rtol) * rn + rt.type(atol)
    out.r0norm, out.target, out.rnorm = float(rn), float(target), float(rn)
    out.status = 0 if np.isfinite(rn) else BREAKDOWN
    margin = _margin(rn, target)
    active = bool(rn > target) and bool(np.isfinite(rn)) and not masked
    steps = 0
    hist = [(x.copy(), float(rn), margin)] if keep_history else None
    p = r.copy()
    if method == "bicgstab":
        rhat = r.copy()
        rho = ct.type(rr)
    else:
        rho = dots(r, r)
    predict = method == "cocg_fused" and rtol >= 1e-3 and atol == 0.0
    tg = target

    def note():
        if keep_history:
            hist.append((x.copy(), float(out.rnorm), margin))

    while active:
        if method == "cocg_fused":
            # k_fused_fin: the true norm of the residual the last vector kernel left (final_check after the last step)
            rn = np.sqrt(rr)
            out.rnorm = float(rn)
            if steps > 0:
                margin = min(margin, _margin(rn, tg))
                if keep_history:
                    hist[-1] = (hist[-1][0], float(rn), margin)
            if not np.isfinite(rn):
                active = False; out.status = BREAKDOWN; break
            if not rn > tg:
                active = False; out.status = 0; break
            if steps >= maxit:
                break
            q = pencil.apply(z, p)
            sigma, kappa = dots(p, q), dots(q, q)
            with np.errstate(all="ignore"):
                al = rho / sigma
            if abs(sigma) == 0 or abs(rho) == 0 or not _finite(al):
                active = False; out.status = BREAKDOWN; break
            rho_next = al * al * kappa - rho
            with np.errstate(all="ignore"):
                beta = rho_next / rho
            steps += 1
            x = x + al * p
            rr_next = abs(rho_next) * (rr / abs(rho))
            stop = False
            if predict:
                margin = min(margin, _margin(rr_next, tg * tg))
                if rr_next <= tg * tg:
                    margin = min(margin, _margin(rr_next, rt.type(1e-12) * rr))
                    stop = bool(rr_next >= rt.type(1e-12) * rr)
            if stop:
                active = False; out.status = 0; out.rnorm = float(np.sqrt(rr_next)); note(); break
            if not _finite(beta):
                active = False; out.status = BREAKDOWN; note(); break
            r = r - al * q
            p = r + beta * p
            rho = dots(r, r)
            rr = dots(r, r, conj=True).real
            out.rnorm = float(np.sqrt(rr))     # (what the norm test that follows reports)
            note()
            continue
        if steps >= maxit:
            break
        if method == "cocg5":
            q = pencil.apply(z, p)
            sigma = dots(p, q)
        else:
            v = pencil.apply(z, p)
            sigma = dots(rhat, v, conj=True)
        with np.errstate(all="ignore"):
            al = rho / sigma                           # k_fin_alpha
        if abs(sigma) == 0 or not _finite(al):
            active = False; out.status = BREAKDOWN; break
        if method == "cocg5":
            x = x + al * p                             # k_cocg_update
            r = r - al * q
            rho_new = dots(r, r)
        else:
            s = r - al * v                             # k_s_update
            t = pencil.apply(z, s)
            ts, tt = dots(t, s, conj=True), dots(t, t, conj=True).real
            with np.errstate(all="ignore"):
                om = ts / tt                           # k_fin_omega
            if tt == 0 or not _finite(om):
                om = ct.type(0)
            x = x + al * p + om * s                    # k_xr_update
            r = s - om * t
            rho_new = dots(rhat, r, conj=True)
        rr = dots(r, r, conj=True).real
        # k_fin_rho
        rn = np.sqrt(rr)
        out.rnorm = float(rn)
        steps += 1
        margin = min(margin, _margin(rn, tg))
        note()
        if not np.isfinite(rn):
            active = False; out.status = BREAKDOWN; break
        if not rn > tg:
            active = False; out.status = 0; break
        with np.errstate(all="ignore"):
            beta = rho_new / rho
            bad = abs(rho) == 0
            if method == "bicgstab":
                beta = beta * (al / om)
                bad = bad or abs(om) == 0
        if bad or not _finite(beta):
            active = False; out.status = BREAKDOWN; break
        rho = rho_new
        if method == "cocg5":
            p = r + beta * p                           # k_cocg_p
        else:
            p = r + beta * (p - om * v)                # k_p_update
    out.x, out.steps, out.active, out.margin, out.history = x, steps, active, margin, hist
    return out


def truncated(col, k):
    """What ``col`` (solved with keep_history and maxit >= k) would have been with maxit = k:
    (x, steps, status, active, margin)."""
    if col.steps <= k:
        return col.x, col.steps, col.status, col.active, col.margin
    x, _, margin = col.history[k]
    return x, k, 0, True, margin


def node_status(cols, rtol, atol):
    """The per-node status that fh_collect_columns (rule FH_FAIL_STOP_TEST) reports at the end of fh_krylov."""
    st = 0
    for c in cols:
        if c.active or not np.isfinite(c.rnorm):
            st = NO_CONVERGENCE
        elif c.status == BREAKDOWN and not (c.rnorm <= atol + rtol * c.r0norm):
            st = NO_CONVERGENCE
    return st


class Sweep:
    """out: [Re] sum_e scale w_e Y_e (N x ncols, float64 complex); steps[node][col]; status[node]; margin[node][col];
    cols[node][col]: the Column records."""
    __slots__ = ("out", "steps", "status", "margin", "cols")


def sweep(A, B, Q, Z, W, scale, real_part, method, rtol, atol, maxit, ritz=None, mask=None, dtype=np.clongdouble,
          dot_chunks=0, dot_seed=0, columns=None, pencil=None):
    """The image of feasthip_contour_apply for the Krylov solvers: node e solves (z_e B - A) Y_e = B Q column by column from
    the Ritz warm start q_c / (z_e - ritz_c) (ritz given) or from zero; a masked column keeps its start.  ``columns``:
    the columns of Q to solve (default all); the arrays returned have one entry per solved column."""
    P = pencil or Pencil(A, B, dtype)
    ct = P.dtype
    dots = Dots(P.N, dot_chunks, dot_seed)
    columns = list(range(Q.shape[1])) if columns is None else list(columns)
    acc = np.zeros((P.N, len(columns)), ct)
    res = Sweep()
    res.cols = []
    for z, w in zip(Z, W):
        row = []
        for j, c in enumerate(columns):
            q = np.asarray(Q[:, c]).astype(ct)
            b = P.mulB(q)
            x0 = None if ritz is None else q / (ct.type(z) - ct.type(ritz[c]))
            col = solve_column(P, z, b, method, rtol, atol, maxit, x0=x0, masked=bool(mask is not None and not mask[c]),
                               dots=dots)
            acc[:, j] += ct.type(w) * ct.type(scale) * col.x
            row.append(col)
        res.cols.append(row)
    if real_part:
        acc = acc.real.astype(ct)
    res.out = acc
    res.steps = np.array([[c.steps for c in row] for row in res.cols], dtype=np.int64)
    res.margin = np.array([[c.margin for c in row] for row in res.cols])
    res.status = np.array([node_status(row, rtol, atol) for row in res.cols], dtype=np.int64)
    return res


DRIFT_ORDERS = ((0, 0), (7, 1), (64, 2), (256, 3))       # (interleaved chunks, permutation seed) of the four fp64 runs


def rel_dist(x, ref):
    ref = np.asarray(ref)
    d = np.linalg.norm((np.asarray(x).astype(ref.dtype) - ref).astype(np.clongdouble))
    n = np.linalg.norm(ref.astype(np.clongdouble))
    return float(d / n) if n > 0 else float(d)


def block_dist(X, ref):
    """Distance of a summed block to the reference, relative to the reference's largest column norm."""
    ref = np.asarray(ref).astype(np.clongdouble)
    d = np.linalg.norm(np.asarray(X).astype(np.clongdouble) - ref)
    n = np.linalg.norm(ref, axis=0).max()
    return float(d / n) if n > 0 else float(d)


def tolerance(D):
    """The device result must lie within max(32 D, 64 eps) of the long-double reference (D: drift of the restatement
    itself in complex128 over DRIFT_ORDERS)."""
    return max(32.0 * D, 64.0 * np.finfo(np.float64).eps)
