"""Per-column restatement of the shifted COCG sweep of csrc/fh_api.hip (fh_shifted_cocg) and csrc/fh_sparse.hip
(k_shift_init, k_shift_fin, k_shift_vec), numpy only.  Pencil and Dots are those of krylov_reference.py, the arithmetic
type is a parameter in the same way (np.clongdouble: the reference proper, np.complex128: the drift measurement).

One column of a B = I problem, all nodes of the family at once.  The start residuals are collinear, r_e^0 = f_e src
(zero guess: src = q, f = 1; Ritz warm start: src = A q - lambda q, f_e = 1 / (z_e - lambda)).  The seed is the node with
the smallest |Im z_e| (ties: the lowest index); r, q = S_seed p_seed and the dots belong to it.  In the kernels' order:

  start     r = src f_seed, p_e = src f_e (p_seed = r); rho = r^T r, |r|^2.
  finalize  |r| = sqrt(|r|^2).  First iteration: pi_e = f_seed / f_e (seed: 1), pi_e_old = pi_e, |r_e^0| = |r| / |pi_e|,
            target_e = rtol |r_e^0| + atol; a node with |r_e^0| <= target_e, a masked column or a non-finite norm never
            iterates.  Every iterating node: stop (status 0) when not |r| / |pi_e| > target_e, status 8 when that norm is not
            finite.  Seed scalars alpha = rho / sigma (sigma = p^T q), rho' = alpha^2 kappa - rho (kappa = q^T q),
            beta = rho' / rho; sigma == 0, rho == 0 or a non-finite alpha: status 8 for every node still iterating; a
            non-finite beta: the step is taken with beta = 0, then status 8.  Per node still iterating
                pi' = (1 + alpha sigma_e) pi + (beta_old alpha / alpha_old)(pi - pi_old)     (sigma_e = z_e - z_seed)
                alpha_e = alpha (pi / pi'),  beta_e = beta (pi / pi')^2,  1 / pi'
            (seed: pi' = 1, alpha, beta exactly); pi' == 0 or a non-finite result: status 8 for that node.
  vector    r -= alpha q; ACC += sum over the stepping nodes, in node order, of (w_e alpha_e) p_e; then
            p_e = r (1 / pi_e') + beta_e p_e for the stepping nodes and, while any node of the column steps, for the seed.
  end       after maxit iterations one more finalize without a step (the stop test on the last residual).
A node that stopped is frozen: pi_e, p_e and its share of ACC stay as they are.
"""
import numpy as np

import krylov_reference as kr

BREAKDOWN = kr.BREAKDOWN


def seed_of(Z):
    im = np.abs(np.asarray(Z).imag)
    return int(np.argmin(im))            # (argmin: the first of equal minima)


class NodeColumn:
    """What one node did on one column.  dx: the correction it added to its start; steps, status (0 / 8), active,
    rnorm (|r| / |pi_e| at its last test), r0norm, target, margin as in krylov_reference.Column."""
    __slots__ = ("dx", "steps", "status", "active", "rnorm", "r0norm", "target", "margin")


def _finite(v):
    return bool(np.isfinite(v.real) and np.isfinite(v.imag))


def solve_family(pencil, Z, src, F, rtol, atol, maxit, masked=False, dots=None, weights=None):
    """-> (list of NodeColumn per node, ACC column = sum_e weights[e] dx_e accumulated in the kernel's order, seed,
    iterations of the seed recurrence that found a live column)."""
    assert pencil.B is None
    ct, rt = pencil.dtype, pencil.real
    dots = dots or kr.Dots(pencil.N)
    Z = [ct.type(z) for z in Z]
    F = [ct.type(f) for f in F]
    n = len(Z)
    W = [ct.type(1)] * n if weights is None else [ct.type(w) for w in weights]
    seed = seed_of(np.array(Z, dtype=np.complex128))
    src = np.asarray(src).astype(ct)
    one = ct.type(1)
    r = src * F[seed]
    p = [r.copy() if e == seed else src * F[e] for e in range(n)]
    rho = dots(r, r)
    rr = dots(r, r, conj=True).real
    out = [NodeColumn() for _ in range(n)]
    for o in out:
        o.dx = np.zeros(pencil.N, ct)
    acc = np.zeros(pencil.N, ct)
    pi = [one] * n
    pio = [one] * n
    active = [False] * n
    alpha_old = beta_old = None
    passes = 0
    for k in range(maxit + 1):
        final = k == maxit
        first = k == 0
        if not first and not any(active):
            break
        rn = np.sqrt(rr)
        flag = 1
        al = beta = fac = ct.type(0)
        if not np.isfinite(rn):
            flag = 3
        elif final:
            flag = 0
        if not final:
            passes += 1
            q = pencil.apply(Z[seed], p[seed])
            sigma, kappa = dots(p[seed], q), dots(q, q)
        if flag == 1:
            with np.errstate(all="ignore"):
                al = rho / sigma
            if abs(sigma) == 0 or abs(rho) == 0 or not _finite(al):
                flag = 2
            else:
                rho_next = al * al * kappa - rho
                with np.errstate(all="ignore"):
                    beta = rho_next / rho
                if not _finite(beta):
                    flag, beta = 4, ct.type(0)
                if not first:
                    fac = beta_old * al / alpha_old
        stepped = [False] * n
        coef = [None] * n
        ipi = [one] * n
        be = [beta] * n
        for e in range(n):
            o = out[e]
            if first:
                pi[e] = one if e == seed else F[seed] / F[e]
                pio[e] = pi[e]
                r0 = rn / abs(pi[e])
                target = rt.type(rtol) * r0 + rt.type(atol)
                o.r0norm, o.target, o.rnorm = float(r0), target, float(r0)
                o.steps, o.margin = 0, kr._margin(r0, target)
                active[e] = bool(r0 > target) and bool(np.isfinite(r0)) and not masked
                o.status = 0 if np.isfinite(r0) else BREAKDOWN
            if not active[e]:
                continue
            rne = rn / abs(pi[e])
            o.rnorm = float(rne)
            if not first:
                o.margin = min(o.margin, kr._margin(rne, o.target))
            if flag == 3 or not np.isfinite(rne):
                active[e] = False; o.status = BREAKDOWN
            elif not rne > o.target:
                active[e] = False; o.status = 0
            elif flag == 2:
                active[e] = False; o.status = BREAKDOWN
            elif flag != 0:
                pin, ae, b_e, ip = one, al, beta, one
                if e != seed:
                    with np.errstate(all="ignore"):
                        pin = (one + al * (Z[e] - Z[seed])) * pi[e] + fac * (pi[e] - pio[e])
                        ratio = pi[e] / pin
                        ae = al * ratio
                        b_e = beta * (ratio * ratio)
                        ip = one / pin
                if abs(pin) == 0 or not (_finite(ae) and _finite(b_e) and _finite(ip)):
                    active[e] = False; o.status = BREAKDOWN
                else:
                    coef[e], ipi[e], be[e] = ae, ip, b_e
                    pio[e], pi[e] = pi[e], pin
                    o.steps += 1
                    stepped[e] = True
                    if flag == 4:
                        active[e] = False; o.status = BREAKDOWN
        if final or not any(stepped):
            continue
        alpha_old, beta_old = al, beta
        r = r - al * q
        rho = dots(r, r)
        rr = dots(r, r, conj=True).real
        tmp = np.zeros(pencil.N, ct)
        for e in range(n):
            if not (stepped[e] or e == seed):
                continue
            if stepped[e]:
                out[e].dx = out[e].dx + coef[e] * p[e]
                tmp = tmp + (W[e] * coef[e]) * p[e]
                p[e] = r * ipi[e] + be[e] * p[e]
            else:
                p[e] = r * one + beta * p[e]
        acc = acc + tmp
    for e in range(n):
        out[e].active = active[e]
        out[e].target = float(out[e].target)
    return out, acc, seed, passes


def start_of(pencil, q, Z, ritz_c):
    """(src, F, x0 per node) of the shared start of column q in the pencil's arithmetic."""
    ct = pencil.dtype
    q = np.asarray(q).astype(ct)
    if ritz_c is None:
        return q, [ct.type(1)] * len(Z), [np.zeros(pencil.N, ct) for _ in Z]
    lam = pencil.real.type(ritz_c)
    src = pencil.mulA(q) - lam * q
    F = [ct.type(1) / (ct.type(z) - lam) for z in Z]
    return src, F, [q * f for f in F]


def sweep(A, Q, Z, W, scale, rtol, atol, maxit, ritz=None, mask=None, dtype=np.clongdouble, dot_chunks=0, dot_seed=0,
          columns=None, pencil=None):
    """The image of feasthip_contour_apply under FEASTHIP_SOLVER_SHIFTED_COCG on an eligible problem, in the layout of
    krylov_reference.sweep: out (complex projection; take .real for the real one), steps[node][col], status[node],
    margin[node][col], cols[node][col], plus seed and passes (per compared column)."""
    P = pencil or kr.Pencil(A, None, dtype)
    ct = P.dtype
    dots = kr.Dots(P.N, dot_chunks, dot_seed)
    columns = list(range(Q.shape[1])) if columns is None else list(columns)
    res = kr.Sweep()
    out = np.zeros((P.N, len(columns)), ct)
    by_col = []
    passes = []
    wts = [ct.type(w) * ct.type(scale) for w in W]
    for j, c in enumerate(columns):
        src, F, _ = start_of(P, Q[:, c], Z, None if ritz is None else ritz[c])
        cols, acc, seed, npass = solve_family(P, Z, src, F, rtol, atol, maxit, masked=bool(mask is not None and not mask[c]),
                                              dots=dots, weights=wts)
        if ritz is not None:
            # k_sum_finish: Q rho_c + ACC, rho_c = sum_e w_e / (z_e - lambda_c) in node order
            rho = ct.type(0)
            for z, w in zip(Z, wts):
                rho = rho + w / (ct.type(z) - P.real.type(ritz[c]))
            acc = acc + rho * np.asarray(Q[:, c]).astype(ct)
        out[:, j] = acc
        by_col.append(cols)
        passes.append(npass)
    res.cols = [[by_col[j][e] for j in range(len(columns))] for e in range(len(Z))]
    res.out = out
    res.steps = np.array([[c.steps for c in row] for row in res.cols], dtype=np.int64)
    res.margin = np.array([[c.margin for c in row] for row in res.cols])
    res.status = np.array([kr.node_status(row, rtol, atol) for row in res.cols], dtype=np.int64)
    return res, seed_of(np.asarray(Z, dtype=np.complex128)), passes
