"""Nonlinear eigenproblems T(lambda) x = 0 in split form, T(lambda) = sum_k f_k(lambda) A_k, with spectra known in closed form,
built from seeds, for the feast_nonlinear tests.  Every case is a dict(terms [(A_k, f_k)], N, center, radius, lam_all (every known
eigenvalue near the circle), lam_in (those inside, sorted), count, m0), computed once and shared: not to be modified.

delay_case       T = -lambda I + A0 + e^{-tau lambda} A1 with A0 = V diag(d0) V^-1, A1 = V diag(d1) V^-1: the scalar equations
                 lambda = d0_i + d1_i e^{-tau lambda} have the roots d0_i + W_b(tau d1_i e^{-tau d0_i}) / tau over the branches b of
                 the Lambert function, and the branches of one i share the eigenvector V[:, i].
grid_delay_case  the same on the sparse 7-point stencil K of a box grid (workloads._weighted_grid_laplacian, one weight per
                 direction so that the grid eigenvalues kappa are distinct): T = K - lambda I + c e^{-tau lambda} I, roots
                 kappa_i + W_b(tau c e^{-tau kappa_i}) / tau.  variable=True: the last term is a random positive diagonal in place
                 of c I, and there is no closed form.
rational_case    K - lambda M + lambda / (lambda - s) e e^T with the pole s outside the circle; multiplied by (lambda - s) it is
                 a quadratic polynomial, whose companion eigenvalues are the reference.
poly_as_terms    a case of polynomial_cases.make_case posed with f_k = k (the integer shorthand for lambda^k)."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
from scipy.special import lambertw

import polynomial_cases as pc
from feastkit_jl_amd import workloads

NE = 16
FPM3 = 10
BRANCHES = range(-3, 4)
SEEDS = (1, 2, 3)

# (N, circle index) of the dense delay cases; circle 3 is empty at N = 33 (the "nothing inside" case) and is listed apart
DELAY_CIRCLES = [(-1.0 + 0.0j, 0.6), (-2.0 + 0.0j, 0.5), (-1.5 + 0.5j, 0.8), (-0.5 + 1.0j, 0.7)]
DELAY_SIZES = (33, 40, 70)
DELAY_CASES = [(N, c) for N in DELAY_SIZES for c in range(4) if not (N == 33 and c == 3)]
DELAY_IDS = ["N%d-circle%d" % nc for nc in DELAY_CASES]
EMPTY_CASE = (33, 3)
# sparse grid cases: dims -> (c, tau, centre, radius); the circles sit at the low end of the grid spectrum
GRID_WEIGHTS = (1.0, 0.7, 0.45)
GRID_CASES = {(6, 5, 4): (-0.5, 1.0, 0.55 + 0.0j, 0.35), (12, 10, 8): (-0.5, 1.0, 0.2 + 0.0j, 0.22)}
GRID_IDS = ["6x5x4", "12x10x8"]


# The seed of the delay matrices was picked on the numpy restatement (nonlinear_reference.driver), the way
# polynomial_cases.CASE_SEEDS were: the first seed of 0 .. 119 under which circle 3 is empty at N = 33 and not at N = 40 and 70,
# some circle holds eigenvalues that share an eigenvector, and the restatement finds exactly the eigenvalues inside every other
# circle from the start seeds 1 .. 3 within the default loop limit (12 loops at most; 10 of the 24 seeds with an empty circle did).
# The seeds that fail do so in two ways, both properties of the method and not of an implementation: an eigenvalue just outside
# the circle makes the 16-node filter converge too slowly for 20 loops, or a spurious candidate of the reduced problem with a
# backward error below POLY_SET_ASIDE[0] stays inside the circle.
DELAY_SEED = 19


def m0_rule(count):
    return max(6, int(1.5 * count) + 2)


def exp_term(tau):
    return lambda z: np.exp(-tau * np.asarray(z, dtype=np.complex128))


def _minus_lambda(z):
    return -np.asarray(z, dtype=np.complex128)


def _one(z):
    return np.ones_like(np.asarray(z, dtype=np.complex128))


def _lambert_roots(d0, d1, tau):
    """the roots of lambda = d0_i + d1_i e^{-tau lambda} over BRANCHES, [i, b]"""
    arg = tau * np.asarray(d1, dtype=np.complex128) * np.exp(-tau * np.asarray(d0, dtype=np.complex128))
    roots = np.stack([np.asarray(d0) + lambertw(arg, b) / tau for b in BRANCHES], axis=1)
    resid = np.abs(roots - np.asarray(d0)[:, None] - np.asarray(d1)[:, None] * np.exp(-tau * roots))
    ok = np.isfinite(roots) & (resid <= 1e-9 * (1.0 + np.abs(roots)))      # (W_b(0) is -inf off the principal branch)
    return roots, ok


def _finish(case, center, radius, lam_all):
    lam_all = np.asarray(lam_all, dtype=np.complex128)
    inside = lam_all[np.abs(lam_all - center) <= radius]
    case.update(center=complex(center), radius=float(radius), lam_all=lam_all, lam_in=np.sort_complex(inside), count=len(inside),
                m0=m0_rule(len(inside)))
    return case


@functools.lru_cache(maxsize=None)
def _delay_matrices(N, tau, seed):
    rng = np.random.default_rng([seed, N, 7])
    V = rng.standard_normal((N, N)) + 3.0 * np.eye(N)
    d0 = -rng.uniform(0.2, 4.0, N)
    d1 = rng.uniform(-1.5, 1.5, N)
    Vi = np.linalg.inv(V)
    roots, ok = _lambert_roots(d0, d1, tau)
    return np.asfortranarray((V * d0) @ Vi), np.asfortranarray((V * d1) @ Vi), roots, ok, V


@functools.lru_cache(maxsize=None)
def delay_case(N, circle, tau=1.0, seed=DELAY_SEED):
    A0, A1, roots, ok, V = _delay_matrices(N, tau, seed)
    center, radius = DELAY_CIRCLES[circle]
    case = {"terms": [(np.asfortranarray(np.eye(N)), _minus_lambda), (A0, _one), (A1, exp_term(tau))], "N": N, "V": V, "roots": roots,
            "roots_ok": ok, "sparse": False}
    return _finish(case, center, radius, roots[ok])


def shared_vector_count(case):
    """how many eigenvalues inside the circle share their eigenvector with another one inside"""
    inside = case["roots_ok"] & (np.abs(case["roots"] - case["center"]) <= case["radius"])
    per = inside.sum(axis=1)
    return int(per[per > 1].sum())


@functools.lru_cache(maxsize=None)
def grid_matrix(dims):
    shape = dims[::-1]
    weights = []
    for d in range(3):
        ax = 2 - d
        s = list(shape)
        s[ax] += 1
        weights.append(np.full(s, GRID_WEIGHTS[d]))
    K = workloads._weighted_grid_laplacian(dims, weights).tocsr()
    kap = np.zeros(1)
    for d in range(3):
        k1 = GRID_WEIGHTS[d] * (2.0 - 2.0 * np.cos(np.pi * np.arange(1, dims[d] + 1) / (dims[d] + 1)))
        kap = (kap[:, None] + k1[None, :]).ravel()
    return K, np.sort(kap)


@functools.lru_cache(maxsize=None)
def grid_delay_case(dims, variable=False, seed=20260802):
    c, tau, center, radius = GRID_CASES[dims]
    K, kap = grid_matrix(dims)
    N = K.shape[0]
    if variable:
        rng = np.random.default_rng([seed, N])
        last = sp.diags(abs(c) * rng.uniform(0.5, 1.5, N)).tocsr() * np.sign(c)
    else:
        last = (c * sp.identity(N)).tocsr()
    case = {"terms": [(K, _one), (sp.identity(N, format="csr"), _minus_lambda), (last, exp_term(tau))], "N": N, "sparse": True,
            "variable": variable}
    if variable:
        return _finish(case, center, radius, np.zeros(0))
    roots, ok = _lambert_roots(kap, np.full(N, c), tau)
    return _finish(case, center, radius, roots[ok])


@functools.lru_cache(maxsize=None)
def rational_case(N=40, seed=20260803):
    rng = np.random.default_rng([seed, N])
    K = np.diag(2.0 * np.ones(N)) - np.diag(np.ones(N - 1), 1) - np.diag(np.ones(N - 1), -1)
    K = K + (0.05j / np.sqrt(N)) * rng.standard_normal((N, N))
    M = np.eye(N) + (0.1 / np.sqrt(N)) * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
    e = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(N)
    E = np.outer(e, e)
    s = 1.6 + 0.4j
    center, radius = 0.5 + 0.0j, 0.6
    terms = [(np.asfortranarray(K), _one), (np.asfortranarray(M), _minus_lambda),
             (np.asfortranarray(E), lambda z: np.asarray(z, dtype=np.complex128) / (np.asarray(z, dtype=np.complex128) - s))]
    # (lambda - s) T(lambda) = -s K + lambda (K + s M + E) - lambda^2 M
    A0, A1, A2 = -s * K, K + s * M + E, -M
    Al = np.block([[np.zeros((N, N)), np.eye(N)], [-A0, -A1]])
    Bl = np.block([[np.eye(N), np.zeros((N, N))], [np.zeros((N, N)), A2]])
    lam = sla.eigvals(Al, Bl)
    lam = lam[np.isfinite(lam)]
    return _finish({"terms": terms, "N": N, "sparse": False, "pole": s}, center, radius, lam)


def poly_as_terms(case):
    """a polynomial_cases case as a split form with f_k = k"""
    out = {"terms": [(Ak, k) for k, Ak in enumerate(case["coeffs"])], "N": case["N"], "sparse": False}
    return _finish(out, case["center"], case["radius"], case["lam_all"])


def dense_terms(terms):
    return [(np.asfortranarray(A.toarray()) if sp.issparse(A) else A, f) for A, f in terms]


def random_terms(N, nterms, cplx, seed=20260804):
    """nterms Gaussian matrices of unit 2-norm order with smooth scalar functions (primitive-level tests: any split form will do)"""
    mats = pc.random_coeffs(N, nterms - 1, cplx, seed)
    funcs = [_one, _minus_lambda, exp_term(0.7), lambda z: 1.0 / (np.asarray(z, dtype=np.complex128) - 9.0), lambda z: np.asarray(z, dtype=np.complex128) ** 2,
             exp_term(-0.3), lambda z: np.sqrt(np.asarray(z, dtype=np.complex128) + 5.0), lambda z: np.sin(np.asarray(z, dtype=np.complex128)),
             lambda z: np.asarray(z, dtype=np.complex128) ** 3]
    return list(zip(mats, funcs[:nterms]))
