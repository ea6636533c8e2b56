"""numpy restatement of the polynomial driver: the first companion form, the structured shifted solve that never forms it,
the contour sum on the explicit companion, and the refinement loop of feast_hip_polynomial."""
import functools
import math

import numpy as np
import scipy.linalg as sla

import feast_oracle as fo
import polynomial_cases as pc


def companion(coeffs):
    """(A_lin, B_lin) of the first companion form: identity blocks on the block super-diagonal and -A_0 .. -A_{d-1} in the
    last block row; B_lin = diag(I, .., I, A_d)."""
    d = len(coeffs) - 1
    N = coeffs[0].shape[0]
    A = np.zeros((d * N, d * N), dtype=np.complex128)
    B = np.eye(d * N, dtype=np.complex128)
    for i in range(d - 1):
        A[i * N:(i + 1) * N, (i + 1) * N:(i + 2) * N] = np.eye(N)
    for j in range(d):
        A[(d - 1) * N:, j * N:(j + 1) * N] = -coeffs[j]
    B[(d - 1) * N:, (d - 1) * N:] = coeffs[d]
    return A, B


def poly_at(coeffs, z):
    P = np.array(coeffs[-1], dtype=np.complex128)
    for Ak in coeffs[-2::-1]:
        P = P * z + Ak
    return P


def structured_solve(coeffs, z, R, lu=None):
    """(z B_lin - A_lin)^-1 R through one N x N solve with P(z):
       D_p = sum_{k=0}^{min(d-2, d-1-p)} A_{k+1+p} R_k,  P(z) Y_0 = R_{d-1} + sum_p z^p D_p,  Y_{i+1} = z Y_i - R_i."""
    d = len(coeffs) - 1
    N = coeffs[0].shape[0]
    Rb = [R[i * N:(i + 1) * N] for i in range(d)]
    rhs = np.array(Rb[d - 1], dtype=np.complex128)
    for p in range(d):
        for k in range(0, min(d - 2, d - 1 - p) + 1):
            rhs = rhs + (z ** p) * (coeffs[k + 1 + p] @ Rb[k])
    if lu is None:
        lu = sla.lu_factor(poly_at(coeffs, z))
    Y = [sla.lu_solve(lu, rhs)]
    for i in range(d - 1):
        Y.append(z * Y[i] - Rb[i])
    return np.vstack(Y)


def contour_sum(coeffs, Zne, Wne, Q):
    """sum_e w_e (z_e B_lin - A_lin)^-1 B_lin Q on the explicit companion -> (sum, condition numbers of the shifted matrices)."""
    A, B = companion(coeffs)
    out = np.zeros_like(Q, dtype=np.complex128)
    conds = []
    BQ = B @ Q
    for z, w in zip(Zne, Wne):
        S = z * B - A
        conds.append(np.linalg.cond(S))
        out += w * np.linalg.solve(S, BQ)
    return out, np.array(conds)


def backward_error(coeffs, lam, X0):
    """||P(lam_j) x_j|| / (sum_k |lam_j|^k ||A_k||_F ||x_j||) per column."""
    fro = [np.linalg.norm(c) for c in coeffs]
    out = np.zeros(len(lam))
    for j, l in enumerate(lam):
        r = poly_at(coeffs, l) @ X0[:, j]
        out[j] = np.linalg.norm(r) / (sum(abs(l) ** k * f for k, f in enumerate(fro)) * np.linalg.norm(X0[:, j]))
    return out


def driver(coeffs, center, radius, M0, ne=pc.NE, fpm3=pc.FPM3, fpm4=20, Q0=None, residual="pencil", seed=20260515):
    """The loop of feast_hip_polynomial (feast_gegv! on the linearisation with M0 d columns) with structured solves."""
    d = len(coeffs) - 1
    N = coeffs[0].shape[0]
    cols = M0 * d
    A, B = companion(coeffs)
    Zne, Wne = fo.feast_gcontour(center, radius, ne)
    Q = fo.seeded_subspace(d * N, cols, seed) if Q0 is None else np.array(Q0, dtype=np.complex128)
    eps_tol = fo.feast_tolerance(fpm3)
    lus = [sla.lu_factor(poly_at(coeffs, z)) for z in Zne]
    loop, hist = 0, []
    while True:
        BQ = B @ Q
        q = np.zeros_like(Q)
        for e, z in enumerate(Zne):
            q += Wne[e] * structured_solve(coeffs, z, BQ, lus[e])
        Sq = q.conj().T @ (B @ q)
        Aq = q.conj().T @ (A @ q)
        lam_red, v_red = sla.eig(Aq, Sq)
        ins = [i for i in range(cols) if fo.inside_gcontour(lam_red[i], center, radius)]
        M = len(ins)
        if M == 0:
            return {"info": 5, "M": 0, "loop": loop, "eps_hist": hist}
        perm = ins + [i for i in range(cols) if i not in set(ins)]
        X = (q @ v_red)[:, perm]
        lam = lam_red[perm]
        X = X / np.linalg.norm(X, axis=0)
        AX, BX = A @ X[:, :M], (B @ X[:, :M] if residual == "pencil" else X[:, :M])
        res = np.array([np.linalg.norm(AX[:, j] - lam[j] * BX[:, j]) / max(abs(lam[j]), 1.0) for j in range(M)])
        epsout = float(res.max())
        hist.append(epsout)
        if epsout <= eps_tol or loop >= fpm4:
            order = sorted(range(M), key=lambda i: abs(lam[i]) ** 2)
            lam_o, X_o = lam[:M][order], X[:N, :M][:, order]
            return {"info": 0, "M": M, "loop": loop, "epsout": epsout, "eps_hist": hist, "lam": lam_o, "q": X_o, "res": res[order],
                    "backward_error": backward_error(coeffs, lam_o, X_o)}
        loop += 1
        Q = X


@functools.lru_cache(maxsize=None)
def driver_run(params, residual="pencil", fpm4=20):
    """The restatement on a driver case of polynomial_cases (computed once, shared, not to be modified)."""
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    return driver(case["coeffs"], case["center"], case["radius"], M0, residual=residual, fpm4=fpm4)


def match_error(found, expected):
    """max over `found` of the distance to the nearest entry of `expected` (and every expected value is used once)."""
    left = list(expected)
    worst = 0.0
    for l in found:
        j = int(np.argmin([abs(l - e) for e in left]))
        worst = max(worst, abs(l - left[j]))
        left.pop(j)
    return worst
