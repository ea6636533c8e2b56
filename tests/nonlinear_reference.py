"""numpy restatement of feast_nonlinear (hip_backend.feast_hip_nonlinear): FEAST for T(lambda) x = 0, T = sum_k f_k(lambda) A_k, on
an N-row subspace with a residual-inverse contour step.  T(z_e) is solved with numpy.linalg.solve, the subspace is
orthonormalised by the oracle's pivoted-QR rank compression (the rank rule of polynomial_projected_reference), the reduced r x r
problem is solved by Beyn's integral method with `moments` block moments and polished by a guarded Newton iteration, and the
selection and set-aside rules are polynomial_projected_reference.select's, with the thresholds read from the package.

The two host rules, restated:
  Beyn     trapezoid rule with `reduced_nodes` points on the caller's circle in the scaled variable u = (z - c) / rho; block moments
           M_p = (1 / n) sum_j u_j^{p+1} That(z_j)^-1, p = 0 .. 2K-1 (full identity as probe); block Hankel matrices H0 = [M_{i+j}],
           H1 = [M_{i+j+1}], K r x K r; SVD of H0 truncated at BEYN_RANK_TOL s_max (and nothing at all is returned when s_max itself is
           below BEYN_NOISE max_j ||That(z_j)^-1||_F: the moments of an empty circle are what is left of the cancelling sum); eigenvalues of U0^H H1 V0 S0^-1 mapped back; the
           first r rows of U0 S are the vectors.
  Newton   at most NEWTON_STEPS steps on the bordered system [That(theta), That'(theta) v; v^H, 0], That' a central difference of the
           f_k with step NEWTON_FD max(1, |theta|); the polished pair is accepted only if it stayed finite and within NEWTON_REACH
           radius of its start AND (reached a reduced backward error <= NEWTON_DONE or ended with a smaller reduced residual than
           it began with); otherwise the Beyn pair is kept."""
import functools
import math

import numpy as np

import feast_oracle as fo
import nonlinear_cases as nc
import polynomial_projected_reference as ppr
from feastkit_jl_amd.hip_backend import BEYN_NOISE, BEYN_RANK_TOL, NEWTON_DONE, NEWTON_FD, NEWTON_REACH, NEWTON_STEPS

RANK_TOL = ppr.RANK_TOL


def as_function(f):
    if callable(f):
        return f
    p = int(f)
    return lambda z: np.asarray(z, dtype=np.complex128) ** p


def table(funcs, z):
    """F[i, k] = f_k(z_i)"""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    with np.errstate(all="ignore"):
        return np.stack([np.asarray(f(z), dtype=np.complex128) * np.ones(z.shape) for f in funcs], axis=1)


def split(terms):
    mats = [np.asarray(A.toarray() if hasattr(A, "toarray") else A) for A, _ in terms]
    return mats, [as_function(f) for _, f in terms]


def t_at(mats, frow):
    return sum(f * A for f, A in zip(frow, mats))


def eval_cols(mats, F, X):
    """R[:, j] = sum_k F[j, k] A_k X[:, j]"""
    R = np.zeros(X.shape, dtype=np.complex128)
    for k, Ak in enumerate(mats):
        R += Ak @ (X * F[None, :, k])
    return R


def sweep(mats, F_node, Zne, Wne, X, sigma=None, F_sigma=None):
    X = np.asarray(X, dtype=np.complex128)
    Q = np.zeros_like(X)
    R = X if sigma is None else eval_cols(mats, F_sigma, X)
    for e, (z, w) in enumerate(zip(Zne, Wne)):
        Y = np.linalg.solve(t_at(mats, F_node[e]), R)
        Q += w * Y if sigma is None else (w / (z - np.asarray(sigma)))[None, :] * (X - Y)
    return Q


def candidate_errors(mats, F_theta, X):
    """be_i = ||sum_k F[i, k] A_k x_i|| / sum_k |F[i, k]| ||A_k||_F for unit x_i; +inf for a non-finite row"""
    fro = np.array([np.linalg.norm(A) for A in mats])
    ok = np.isfinite(F_theta).all(axis=1)
    F = np.where(ok[:, None], F_theta, 0.0)
    num = np.linalg.norm(eval_cols(mats, F, X), axis=0)
    with np.errstate(all="ignore"):
        be = num / (np.abs(F) @ fro)
    be[~ok | ~np.isfinite(be)] = np.inf
    return be


def beyn(Ahat, funcs, center, radius, moments, reduced_nodes):
    """-> (theta[ncand], Y[r, ncand]) of the reduced problem inside (and just outside) the circle"""
    r = Ahat[0].shape[0]
    K, n = int(moments), int(reduced_nodes)
    u = np.exp(2j * np.pi * (np.arange(n) + 0.5) / n)
    F = table(funcs, center + radius * u)
    Mp = np.zeros((2 * K, r, r), dtype=np.complex128)
    scale = 0.0
    for j in range(n):
        Tinv = np.linalg.inv(t_at(Ahat, F[j]))
        scale = max(scale, np.linalg.norm(Tinv))
        for p in range(2 * K):
            Mp[p] += (u[j] ** (p + 1) / n) * Tinv
    H0 = np.block([[Mp[i + j] for j in range(K)] for i in range(K)])
    H1 = np.block([[Mp[i + j + 1] for j in range(K)] for i in range(K)])
    U, s, Vh = np.linalg.svd(H0)
    k = int(np.sum(s > BEYN_RANK_TOL * s[0])) if s[0] > BEYN_NOISE * scale else 0
    if k == 0:
        return np.zeros(0, dtype=np.complex128), np.zeros((r, 0), dtype=np.complex128)
    U0, V0 = U[:, :k], Vh[:k].conj().T
    B = (U0.conj().T @ H1 @ V0) / s[None, :k]
    mu, S = np.linalg.eig(B)
    return center + radius * mu, (U0 @ S)[:r]


def reduced_error(Ahat, fro, funcs, theta, v):
    """(||That(theta) v||, that over sum_k |f_k(theta)| ||Ahat_k||_F) for unit v"""
    f = table(funcs, theta)[0]
    if not np.isfinite(f).all():
        return math.inf, math.inf
    res = float(np.linalg.norm(t_at(Ahat, f) @ v))
    den = float(np.abs(f) @ fro)
    return res, (res / den if den > 0 else math.inf)


def newton_polish(Ahat, funcs, theta0, v0, radius):
    """the guarded Newton polish of one Beyn pair -> (theta, v)"""
    fro = np.array([np.linalg.norm(A) for A in Ahat])
    r = len(v0)
    nv = np.linalg.norm(v0)
    if not (np.isfinite(theta0) and nv > 0 and np.isfinite(nv)):
        return theta0, v0
    v0 = v0 / nv
    res0, be0 = reduced_error(Ahat, fro, funcs, theta0, v0)
    theta, v, res, be = theta0, v0, res0, be0
    for _ in range(NEWTON_STEPS):
        if not be > NEWTON_DONE:
            break
        h = NEWTON_FD * max(1.0, abs(theta))
        F = table(funcs, [theta, theta + h, theta - h])
        if not np.isfinite(F).all():
            return theta0, v0
        T = t_at(Ahat, F[0])
        dT = t_at(Ahat, (F[1] - F[2]) / (2.0 * h))
        Jb = np.zeros((r + 1, r + 1), dtype=np.complex128)
        Jb[:r, :r] = T
        Jb[:r, r] = dT @ v
        Jb[r, :r] = v.conj()
        rhs = np.zeros(r + 1, dtype=np.complex128)
        rhs[r] = 1.0
        try:
            sol = np.linalg.solve(Jb, rhs)
        except np.linalg.LinAlgError:
            break
        nrm = np.linalg.norm(sol[:r])
        if not (np.isfinite(sol).all() and nrm > 0):
            return theta0, v0
        theta, v = theta + sol[r], sol[:r] / nrm
        res, be = reduced_error(Ahat, fro, funcs, theta, v)
    ok = np.isfinite(theta) and np.isfinite(res) and abs(theta - theta0) <= NEWTON_REACH * radius and (be <= NEWTON_DONE or res < res0)
    return (theta, v) if ok else (theta0, v0)


def reduced_solve(Ahat, funcs, center, radius, moments, reduced_nodes):
    theta, Y = beyn(Ahat, funcs, center, radius, moments, reduced_nodes)
    theta = theta.copy()
    Y = Y.copy()
    for i in range(len(theta)):
        theta[i], Y[:, i] = newton_polish(Ahat, funcs, theta[i], Y[:, i], radius)
    return theta, Y


def driver(terms, center, radius, m0, ne=nc.NE, fpm3=nc.FPM3, fpm4=20, X0=None, seed=20260515, moments=2, reduced_nodes=128, perturb=0.0):
    """The loop of hip_backend.feast_hip_nonlinear -> dict(info, M, lam, q, res, epsout, loop, eps_history, rank, candidates, set_aside)."""
    mats, funcs = split(terms)
    N = mats[0].shape[0]
    Zne, Wne = fo.feast_gcontour(center, radius, ne)
    F_node = table(funcs, Zne)
    X = fo.seeded_subspace(N, m0, seed) if X0 is None else np.array(X0, dtype=np.complex128)
    if perturb:
        rng = np.random.default_rng(99)
        X = X * (1.0 + perturb * rng.standard_normal(X.shape))
    sigma = F_sigma = None
    tol = 10.0 ** -fpm3
    hist, ranks, cands, asides = [], [], [], []
    loop = 0
    empty = {"info": 2, "M": 0, "lam": np.zeros(0, dtype=np.complex128), "q": np.zeros((N, 0), dtype=np.complex128), "res": np.zeros(0),
             "epsout": math.inf, "eps_history": hist, "rank": ranks, "candidates": cands, "set_aside": asides}
    while True:
        Q = sweep(mats, F_node, Zne, Wne, X, sigma, F_sigma)
        nrm = np.linalg.norm(Q, axis=0)
        Q = Q / np.where(nrm > 0, nrm, 1.0)
        Q, r = fo.qr_compress(Q, Q.shape[1], RANK_TOL)
        if r == 0:
            return dict(empty, loop=loop)
        Ahat = [Q.conj().T @ (Ak @ Q) for Ak in mats]
        theta, Y = reduced_solve(Ahat, funcs, center, radius, moments, reduced_nodes)
        ncand = len(theta)
        if ncand == 0:
            hist.append(math.inf); ranks.append(r); cands.append(0); asides.append(0)
            return dict(empty, loop=loop)
        Xc = Q @ Y
        cn = np.linalg.norm(Xc, axis=0)
        Xc = Xc / np.where(cn > 0, cn, 1.0)
        F_theta = table(funcs, theta)
        be = candidate_errors(mats, F_theta, Xc)
        be[~(cn > 0)] = np.inf
        keep = min(m0, ncand)
        sel, good, aside = ppr.select(theta, be, center, radius, keep)
        M = int(good.sum())
        epsout = float(be[sel][good].max()) if M else math.inf
        hist.append(epsout); ranks.append(r); cands.append(ncand); asides.append(aside)
        if (M and epsout <= tol) or loop >= fpm4:
            if M == 0:
                return dict(empty, loop=loop)
            idx = sel[good]
            idx = idx[np.argsort(np.abs(theta[idx]) ** 2, kind="stable")]
            return {"info": 0 if epsout <= tol else 2, "M": M, "lam": theta[idx], "q": Xc[:, idx], "res": be[idx], "epsout": epsout,
                    "loop": loop, "eps_history": hist, "rank": ranks, "candidates": cands, "set_aside": asides}
        X = Xc[:, sel]
        sigma = np.where(np.isfinite(theta[sel]), theta[sel], center)
        F_sigma = table(funcs, sigma)
        loop += 1


def match_error(lam, exact):
    """largest distance from a computed eigenvalue to the nearest exact one, after a one-to-one greedy pairing"""
    left = list(exact)
    worst = 0.0
    for x in lam:
        j = int(np.argmin(np.abs(np.asarray(left) - x)))
        worst = max(worst, abs(left[j] - x))
        left.pop(j)
    return worst


@functools.lru_cache(maxsize=None)
def delay_run(N, circle, seed, moments=2, perturb=0.0):
    case = nc.delay_case(N, circle)
    return driver(case["terms"], case["center"], case["radius"], case["m0"], seed=seed, moments=moments, perturb=perturb)


@functools.lru_cache(maxsize=None)
def grid_run(dims, variable, seed, perturb=0.0):
    case = nc.grid_delay_case(dims, variable)
    m0 = case["m0"] if not variable else nc.grid_delay_case(dims, False)["m0"]
    return driver(case["terms"], case["center"], case["radius"], m0, seed=seed, perturb=perturb)


@functools.lru_cache(maxsize=None)
def rational_run(seed, perturb=0.0):
    case = nc.rational_case()
    return driver(case["terms"], case["center"], case["radius"], case["m0"], seed=seed, perturb=perturb)
