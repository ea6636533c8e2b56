"""numpy restatement of the eigenvalue-count estimate of feast_polynomial / feast_nonlinear (fpm[14] = 2, M0 = "auto").

For a regular T(lambda) = sum_k f_k(lambda) A_k (a polynomial: f_k = lambda^k) the number of eigenvalues inside a contour is
(1 / 2 pi i) oint tr(T(z)^-1 T'(z)) dz, and with the nodes z_e and weights w_e of the contour it becomes
    trace = sum_e w_e tr(T'(z_e) T(z_e)^-1),      T'(z_e) = sum_k g_k(z_e) A_k.
The device samples it with Rademacher columns, t_c = v_c^T [sum_e w_e T'(z_e) T(z_e)^-1 v_c].  Everything here is dense numpy on
the host: the tables F[e, k] = f_k(z_e) and G[e, k] = w_e g_k(z_e), the exact trace, the samples for a given block V, their mean
and standard error, and the two M0 rules."""
import math

import numpy as np
import scipy.sparse as sp

FD_STEP = 1e-6          # central-difference step of the f_k, relative to max(1, |z|)


def dense(mats):
    return [np.asarray(A.toarray()) if sp.issparse(A) else np.asarray(A) for A in mats]


def as_functions(funcs):
    """callables of a split form; a non-negative int p stands for lambda^p"""
    return [f if callable(f) else (lambda z, p=int(f): np.asarray(z, dtype=np.complex128) ** p) for f in funcs]


def poly_tables(degree, Z, W):
    """(F, G) of a polynomial: F[e, k] = z_e^k, G[e, k] = w_e k z_e^(k-1)"""
    Z, W = np.asarray(Z, dtype=np.complex128), np.asarray(W, dtype=np.complex128)
    F = np.stack([Z ** k for k in range(degree + 1)], axis=1)
    G = np.stack([W * (k * Z ** (k - 1) if k else 0.0) for k in range(degree + 1)], axis=1)
    return F, G


def term_tables(funcs, Z, W):
    """(F, G) of a split form: F[e, k] = f_k(z_e), G[e, k] = w_e (f_k(z_e + h) - f_k(z_e - h)) / 2h, h = FD_STEP max(1, |z_e|)"""
    funcs = as_functions(funcs)
    Z, W = np.asarray(Z, dtype=np.complex128), np.asarray(W, dtype=np.complex128)
    h = FD_STEP * np.maximum(1.0, np.abs(Z))
    F = np.stack([np.asarray(f(Z), dtype=np.complex128) * np.ones(len(Z)) for f in funcs], axis=1)
    D = np.stack([(np.asarray(f(Z + h), dtype=np.complex128) - np.asarray(f(Z - h), dtype=np.complex128)) / (2.0 * h) * np.ones(len(Z))
                  for f in funcs], axis=1)
    return F, W[:, None] * D


def _combine(mats, row):
    return sum(c * A for c, A in zip(row, mats))


def exact_trace(mats, F, G):
    """sum_e tr((sum_k G[e, k] A_k) (sum_k F[e, k] A_k)^-1) on dense matrices"""
    mats = dense(mats)
    tr = 0.0 + 0.0j
    for e in range(F.shape[0]):
        tr += np.trace(np.linalg.solve(_combine(mats, F[e]).T, _combine(mats, G[e]).T))      # tr(T' T^-1) = tr(T^-T T'^T)
    return complex(tr)


def samples(mats, F, G, V):
    """(t, cond): t[c] = v_c^T [sum_e (sum_k G[e, k] A_k) T(z_e)^-1 v_c] for the columns of V, and the largest 2-norm condition
    number of the T(z_e)"""
    mats = dense(mats)
    acc = np.zeros(V.shape, dtype=np.complex128)
    cond = 0.0
    for e in range(F.shape[0]):
        T = _combine(mats, F[e])
        cond = max(cond, float(np.linalg.cond(T)))
        acc += _combine(mats, G[e]) @ np.linalg.solve(T, V.astype(np.complex128))
    return (V * acc).sum(axis=0), cond


def mean_stderr(t):
    """mean and standard error of the samples as the drivers report them (complex mean; the standard deviation of complex
    samples is that of their moduli about the mean, as numpy defines it)"""
    t = np.asarray(t)
    return complex(np.mean(t)), (float(np.std(t, ddof=1) / math.sqrt(len(t))) if len(t) > 1 else math.inf)


def count(mean):
    return max(0, int(round(float(np.real(mean)))))


def auto_M0(mean, stderr, N):
    """M0 of the projected method and of feast_nonlinear: 1.5 (Re mean + 2 stderr), at least 8, at most N"""
    return int(min(N, max(8, math.ceil(1.5 * (float(np.real(mean)) + 2.0 * float(stderr))))))


def auto_M0_linearised(mean, stderr, N, d):
    """M0 of the linearised method, which runs M0 d columns"""
    return max(1, math.ceil(auto_M0(mean, stderr, N) / d))
