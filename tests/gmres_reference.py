"""Batch-level restatement of the device's restarted GMRES (csrc/fh_gmres.hip: k_gm_start, k_gm_dots / k_gm_fin_h /
k_gm_update, k_gm_givens, k_gm_scale_store, k_gm_solve_y, k_gm_xupdate; the driver fh_gmres in csrc/fh_api.hip), numpy only,
in the style of krylov_reference.py, whose Pencil, Dots, rel_dist, block_dist, tolerance and _margin it reuses.

One call (solve_batch) is one NODE BATCH: the columns of all its nodes advance in lock-step and share one step budget.
The arithmetic type and the order of the dots are parameters (np.clongdouble: the reference proper; np.complex128 over
krylov_reference.DRIFT_ORDERS: the drift measurement).  It follows the device, not a textbook:

  restart     mr = max(restart, 2); target = atol + rtol |r0| with r0 = b - S x0 from the guess in X.
  cycle start the true residual r = b - S x and beta = |r| of every column (one product); a column is active iff beta is
              finite and beta > target; a non-finite beta: status 8.  v_0 = r (1 / beta).
  cap         the batch ends when no column is active or the lock-step counter has reached maxit.  The counter counts the
              lock-steps that ran: a cycle ends after the step in which its last active column left.
  lock-step k w = S v_k; classical Gram-Schmidt twice: h = V^H w, w -= V h, c = V^H w, w -= V c, H[:, k] = h + c,
              h_{k+1,k} = |w| after the second update; the earlier rotations on H[:, k], then (a = H[k,k], b = h_{k+1,k},
              den = sqrt(|a|^2 + |b|^2)): den == 0: (c, s) = (1, 0); |a| == 0: (0, 1); else c = |a| / den (real),
              s = (a / |a|) conj(b) / den; H[k,k] = c a + s b; g_{k+1} = -conj(s) g_k, g_k = c g_k; iters += 1,
              kdim = k + 1, rn = |g_{k+1}|; non-finite rn or h_{k+1,k}: the column leaves with status 8; it leaves when
              !(rn > target) or h_{k+1,k} == 0; v_{k+1} = w (1 / h_{k+1,k}).
  cycle end   y by back substitution over the column's own kdim (a zero diagonal gives y_i = 0), x += sum_i y_i v_i.
  finish      fh_collect_columns under FH_FAIL_TARGET: a node reports 5 when a column is still active at the last cycle
              start, its norm is not finite or above its target.  The reported norm is the last TRUE residual.
  warm start  x0 = q_c / (z_e - ritz_c); the column mask is ignored.
  products    one per cycle start and one per lock-step that ran, per batch (feasthip_stats.spmm_calls).

Exhaustion of the Krylov space (N <= restart, or a right-hand side in an invariant subspace of dimension d): in floating
point h_{d+1,d} is round-off, never 0.0, so neither this restatement nor the device takes the `== 0` branch.  Both stop at
step d because the Givens estimate |g_{d+1}| is then round-off too, far below any target the working precision can
resolve (rtol >= 1e-10 in the pinned cases): the column leaves at step d with status 0 and the iterate is the exact
solution to rounding.  A column that has not reached its target when the space is exhausted (a target below the rounding
level) would go on with v_{d+1} = w / round-off, which is noise in every arithmetic; such a case cannot be pinned and the
cases avoid it (their drift D would break the discriminating-power condition).

Batching never changes what a column computes; it changes only how many lock-steps are left.  In exact arithmetic the
Givens estimate IS the true residual norm, so a column that left on the estimate is never reactivated by the next cycle
start, every column that is active takes every lock-step, and steps and iterates are the same for every batch size.  A
reactivation is a rounding event (estimate and true residual on opposite sides of the target): its margin is of the order
of the rounding level and the column is left undecided.
"""
import numpy as np

from krylov_reference import BREAKDOWN, NO_CONVERGENCE, Dots, Pencil, _margin, block_dist, rel_dist, tolerance  # noqa: F401


class Column:
    """What one (node, column) did.  x: the iterate it ended with; steps: the device's ``iters``; status 0 or 8; active:
    above its target at the last cycle start; rnorm: the last true residual norm; margin: the smallest |lhs/rhs - 1| over
    the stop comparisons evaluated; reactivated: cycle starts that found it above the target after it had left on the
    estimate; history (keep_history: True or the set of t to keep): history[t] = (x_t, steps_t, margin_t) after lock-step
    t of the batch, x_t being what the cycle end would leave if the batch were cut there."""
    __slots__ = ("x", "steps", "status", "active", "rnorm", "r0norm", "target", "margin", "reactivated", "history",
                 "b", "z", "V", "H", "cs", "sn", "g", "w", "inv", "kdim", "left")


class Batch:
    """cols[node][column]; lock_steps: the steps that ran; products: operator applications; cycles: cycle starts."""
    __slots__ = ("cols", "lock_steps", "products", "cycles", "starts", "pencil", "dots", "maxit")


def _multi_dot(dots, V, w):
    """conj(V)^T w, every entry summed in the order of ``dots`` (krylov_reference.Dots)."""
    prod = np.conj(V) * w[:, None]
    if not dots.chunks:
        return prod.sum(axis=0)
    prod = prod[dots.perm]
    n = (prod.shape[0] // dots.chunks) * dots.chunks
    part = prod[:n].reshape(-1, dots.chunks, prod.shape[1]).sum(axis=0)
    part[:prod.shape[0] - n] += prod[n:]
    tot = np.zeros(prod.shape[1], prod.dtype)
    for row in part:
        tot = tot + row
    return tot


def _back_substitute(c, ct):
    kk = c.kdim
    y = np.zeros(kk, ct)
    for i in range(kk - 1, -1, -1):
        s = c.g[i]
        for j in range(i + 1, kk):
            s = s - c.H[i, j] * y[j]
        d = c.H[i, i]
        y[i] = s / d if abs(d) > 0 else ct.type(0)
    return y


def _cycle_x(c, ct, kmax):
    """x + V y over min(kmax, kdim) basis vectors (k_gm_solve_y, k_gm_xupdate)."""
    kk = min(kmax, c.kdim)
    if kk == 0:
        return c.x
    y = _back_substitute(c, ct)
    x = c.x.copy()
    for i in range(kk):
        x = x + y[i] * c.V[:, i]
    return x


def solve_batch(pencil, zs, rhs, x0s, rtol, atol, maxit, restart, dots=None, keep_history=False):
    """zs: the shifts of the batch's nodes; rhs: N x m, shared by the nodes; x0s: per node an N x m guess or None (zero)."""
    P = pencil
    ct, rt = P.dtype, P.real
    N = P.N
    dots = dots or Dots(N)
    mr = max(int(restart), 2)
    rhs = np.asarray(rhs)
    m = rhs.shape[1]
    out = Batch()
    out.pencil, out.dots, out.maxit = P, dots, maxit
    out.cols = []
    for e, z in enumerate(zs):
        row = []
        for j in range(m):
            c = Column()
            c.z = ct.type(z)
            c.b = rhs[:, j].astype(ct)
            c.x = np.zeros(N, ct) if x0s is None or x0s[e] is None else np.asarray(x0s[e])[:, j].astype(ct)
            c.steps, c.status, c.active, c.margin, c.reactivated, c.left = 0, 0, False, np.inf, 0, False
            c.history = {} if keep_history else None
            row.append(c)
        out.cols.append(row)
    allc = [c for row in out.cols for c in row]
    total, products, cycles, first, starts = 0, 0, 0, True, []
    while True:
        # k_gm_start on the residual product (dot_mode 3)
        products += 1
        cycles += 1
        for c in allc:
            r = c.b - P.apply(c.z, c.x)
            beta = np.sqrt(dots(r, r, conj=True).real)
            if first:
                c.r0norm = float(beta)
                c.target = rt.type(atol) + rt.type(rtol) * beta
            c.rnorm = float(beta)
            c.margin = min(c.margin, _margin(beta, c.target))
            fin = bool(np.isfinite(beta))
            c.active = fin and bool(beta > c.target)
            if not fin:
                c.status = BREAKDOWN
            if c.active and c.left:
                c.reactivated += 1
            c.left = False
            c.kdim = 0
            c.inv = rt.type(1) / beta if c.active and beta > 0 else rt.type(0)
            c.w = r
            if c.active:
                c.V = np.zeros((N, mr + 1), ct, order="F")
                c.H = np.zeros((mr + 1, mr), ct)
                c.cs = np.zeros(mr, ct)
                c.sn = np.zeros(mr, ct)
                c.g = np.zeros(mr + 1, ct)
                c.g[0] = beta
                c.V[:, 0] = r * c.inv
        if first and keep_history:
            for c in allc:
                c.history[0] = (c.x.copy(), 0, c.margin)
        first = False
        if not any(c.active for c in allc) or total >= maxit:
            break
        ksteps = 0
        for k in range(mr):
            if total >= maxit or not any(c.active for c in allc):
                break
            for c in allc:
                if not c.active:
                    continue
                Vk = c.V[:, :k + 1]
                w = P.apply(c.z, c.V[:, k])
                h = _multi_dot(dots, Vk, w)                 # first pass
                w = w - Vk @ h
                cc = _multi_dot(dots, Vk, w)                # second pass: the correction, added to H
                w = w - Vk @ cc
                c.H[:k + 1, k] = h + cc
                hk1 = np.sqrt(dots(w, w, conj=True).real)
                Hc = c.H[:, k]
                Hc[k + 1] = hk1
                for i in range(k):                          # k_gm_givens
                    t = c.cs[i] * Hc[i] + c.sn[i] * Hc[i + 1]
                    Hc[i + 1] = -np.conj(c.sn[i]) * Hc[i] + c.cs[i] * Hc[i + 1]
                    Hc[i] = t
                av, bv = Hc[k], Hc[k + 1]
                with np.errstate(all="ignore"):
                    aa = np.sqrt(av.real * av.real + av.imag * av.imag)
                    den = np.sqrt(av.real * av.real + av.imag * av.imag + bv.real * bv.real + bv.imag * bv.imag)
                    if den == 0:
                        c.cs[k], c.sn[k] = 1, 0
                    elif aa == 0:
                        c.cs[k], c.sn[k] = 0, 1
                    else:
                        c.cs[k] = aa / den
                        c.sn[k] = (av * (rt.type(1) / aa)) * np.conj(bv) * (rt.type(1) / den)
                    Hc[k] = c.cs[k] * av + c.sn[k] * bv
                    Hc[k + 1] = 0
                    c.g[k + 1] = -np.conj(c.sn[k]) * c.g[k]
                    c.g[k] = c.cs[k] * c.g[k]
                    rn = abs(c.g[k + 1])
                c.steps += 1
                c.kdim = k + 1
                c.rnorm = float(rn)
                c.margin = min(c.margin, _margin(rn, c.target))
                if not (np.isfinite(rn) and np.isfinite(hk1)):
                    c.active = False
                    c.status = BREAKDOWN
                elif not rn > c.target or hk1 == 0:
                    c.active = False
                    c.left = True
                with np.errstate(all="ignore"):
                    c.inv = rt.type(1) / hk1 if c.active else rt.type(0)
                    c.V[:, k + 1] = w * c.inv
            ksteps += 1
            total += 1
            products += 1
            starts.append(cycles)
            if keep_history is True or (keep_history and total in keep_history):
                for c in allc:
                    c.history[total] = (_cycle_x(c, ct, ksteps), c.steps, c.margin)
        for c in allc:
            c.x = _cycle_x(c, ct, ksteps)
            c.kdim = 0
    for c in allc:
        c.V = c.H = c.cs = c.sn = c.g = c.w = None
    out.lock_steps, out.products, out.cycles, out.starts = total, products, cycles, starts
    return out


def truncated(batch, col, k):
    """What ``col`` of ``batch`` (solved with keep_history and maxit >= k) would have been with maxit = k:
    (x, steps, status, active, margin).  Valid while no column of the batch has a non-finite value.  The cut batch ends
    with one more cycle start: its true residual decides ``active``."""
    if batch.lock_steps <= k:
        return col.x, col.steps, col.status, col.active, col.margin
    x, steps, margin = col.history[k]
    P = batch.pencil
    r = col.b - P.apply(col.z, x)
    beta = np.sqrt(batch.dots(r, r, conj=True).real)
    margin = min(margin, _margin(beta, col.target))
    return x, steps, 0, bool(beta > col.target), margin


def truncated_products(batch, k):
    """spmm_calls of the batch cut at maxit = k: the cycle starts up to lock-step k, the k steps and the closing start."""
    if batch.lock_steps <= k:
        return batch.products
    return batch.starts[k - 1] + k + 1


def node_status(cols):
    """fh_collect_columns under FH_FAIL_TARGET."""
    for c in cols:
        if c.active or not np.isfinite(c.rnorm) or c.rnorm > float(c.target):
            return NO_CONVERGENCE
    return 0


class Sweep:
    """out: [Re] sum_e scale w_e Y_e (N x ncols, complex of the arithmetic); steps[node][col]; status[node];
    margin[node][col]; cols[node][col]: the Column records; products: operator applications of all batches;
    lock_steps: per batch; reactivated: cycle starts that reactivated a column."""
    __slots__ = ("out", "steps", "status", "margin", "cols", "products", "lock_steps", "reactivated")


def sweep(A, B, Q, Z, W, scale, real_part, rtol, atol, maxit, restart, batch=None, ritz=None, mask=None,
          dtype=np.clongdouble, dot_chunks=0, dot_seed=0, columns=None, pencil=None):
    """The image of feasthip_contour_apply with solver GMRES: nodes in batches of ``batch`` (default: all in one), node e
    solves (z_e B - A) Y_e = B Q from the Ritz warm start q_c / (z_e - ritz_c) (ritz given) or from zero.  ``mask`` is
    accepted and ignored, as the device ignores it.  ``columns``: the columns of Q to solve (default all) -- only where
    leaving the others out cannot change the lock-step count (no cap reached)."""
    P = pencil or Pencil(A, B, dtype)
    ct = P.dtype
    dots = Dots(P.N, dot_chunks, dot_seed)
    columns = list(range(Q.shape[1])) if columns is None else list(columns)
    Qc = np.asarray(Q)[:, columns].astype(ct)
    rhs = np.stack([P.mulB(Qc[:, j]) for j in range(len(columns))], axis=1)
    nb = len(Z) if batch is None else int(batch)
    res = Sweep()
    res.cols, res.lock_steps, res.products = [], [], 0
    for e0 in range(0, len(Z), nb):
        zs = list(Z[e0:e0 + nb])
        x0s = None
        if ritz is not None:
            lam = np.asarray(ritz)[columns].astype(P.real)
            x0s = [Qc / (ct.type(z) - lam.astype(ct))[None, :] for z in zs]
        b = solve_batch(P, zs, rhs, x0s, rtol, atol, maxit, restart, dots=dots)
        res.cols += b.cols
        res.lock_steps.append(b.lock_steps)
        res.products += b.products
    acc = np.zeros((P.N, len(columns)), ct)
    for w, row in zip(W, res.cols):
        for j, c in enumerate(row):
            acc[:, j] += ct.type(w) * ct.type(scale) * c.x
    if real_part:
        acc = acc.real.astype(ct)
    res.out = acc
    res.steps = np.array([[c.steps for c in row] for row in res.cols], dtype=np.int64)
    res.margin = np.array([[c.margin for c in row] for row in res.cols])
    res.status = np.array([node_status(row) for row in res.cols], dtype=np.int64)
    res.reactivated = sum(c.reactivated for row in res.cols for c in row)
    return res
