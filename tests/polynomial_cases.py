"""Matrix polynomials with a known spectrum for the polynomial-driver tests.

P(lambda) = C (lambda - X_1) ... (lambda - X_d), X_i = V_i diag(mu_i) V_i^-1 with V_i a random unitary plus 0.15 / sqrt(N)
Gaussian noise (non-normal factors, well conditioned eigenvector bases).  det P(lambda) = det C prod_i det(lambda - X_i), so
the d N eigenvalues are the mu_i: k of them inside the circle, spread over the factors at |lambda - c| <= 0.8 r, the rest at
|lambda - c| in [2.5 r, 4.5 r].  C = I gives a monic polynomial; the non-monic cases take a complex perturbed identity."""
import functools

import numpy as np

CENTER = 0.3 + 0.2j
RADIUS = 1.0
NE = 16            # fpm[8]
FPM3 = 10          # stop at 1e-10: at the default 1e-12 the loop count of these cases depends on rounding

# driver cases: (N, d, k, M0, monic)
DRIVER_CASES = [(70, 2, 6, 6, True), (70, 2, 6, 6, False), (45, 3, 7, 5, True), (45, 3, 7, 5, False), (70, 1, 5, 8, False)]
DRIVER_IDS = ["N%d-d%d-k%d-M0%d-%s" % (N, d, k, M0, "monic" if monic else "nonmonic") for N, d, k, M0, monic in DRIVER_CASES]
# primitive shapes of the sweep / product / residual tests: (N, d, m)
SWEEP_SHAPES = [(70, 2, 12), (45, 3, 15), (193, 2, 72), (45, 8, 15)]
# poly_solve: (N, d, complex coefficients)
SOLVE_SHAPES = [(70, 1, True), (70, 2, True), (45, 3, False), (193, 2, True), (130, 4, True), (45, 8, True)]


def _unitary(rng, N):
    Z = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    Q, R = np.linalg.qr(Z)
    return Q * (np.diag(R) / np.abs(np.diag(R)))


# The loop runs M0 d columns for k < M0 d eigenvalues and never orthonormalises, so it carries M0 d - k junk directions whose
# Ritz values may fall inside the circle and keep epsout at O(1) for a loop (the known weakness of this variant).  The seeds of
# the driver cases were picked on the numpy restatement (polynomial_reference.driver) so that it stops at loop 2 with the
# residual history clear of the threshold on both sides (loop 1: 7e-9 .. 7e-8, loop 2: <= 3e-11), and does so unchanged under
# 1e-14 relative perturbations of the start block and 1e-15 of the coefficients: the loop count then does not hang on rounding.
CASE_SEEDS = {(70, 2, 6, True): 3, (70, 2, 6, False): 5, (45, 3, 7, True): 4, (45, 3, 7, False): 28, (70, 1, 5, False): 1}


def make_case(N, d, k, monic, seed=None):
    """-> dict(coeffs [A_0 .. A_d], N, d, k, lam_in (k values inside), lam_all (d N), center, radius).  Computed once per case
    and shared: not to be modified."""
    return _make_case(N, d, k, monic, CASE_SEEDS.get((N, d, k, monic), 20260601) if seed is None else seed)


@functools.lru_cache(maxsize=None)
def _make_case(N, d, k, monic, seed):
    rng = np.random.default_rng([seed, N, d, k, int(monic)])
    counts = [k // d + (1 if i < k % d else 0) for i in range(d)]
    golden = np.pi * (3.0 - np.sqrt(5.0))
    inside = CENTER + 0.8 * RADIUS * np.sqrt((np.arange(k) + 0.5) / k) * np.exp(1j * golden * np.arange(k))
    inside = inside[rng.permutation(k)]
    poly = [np.eye(N, dtype=np.complex128)] if monic else \
        [np.eye(N) + (0.2 / np.sqrt(N)) * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))]
    lam_all, off = [], 0
    for i in range(d):
        mu = np.empty(N, dtype=np.complex128)
        mu[:counts[i]] = inside[off:off + counts[i]]
        off += counts[i]
        nout = N - counts[i]
        mu[counts[i]:] = CENTER + RADIUS * rng.uniform(2.5, 4.5, nout) * np.exp(2j * np.pi * rng.uniform(0, 1, nout))
        V = _unitary(rng, N) + (0.15 / np.sqrt(N)) * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)))
        X = (V * mu) @ np.linalg.inv(V)
        # poly <- poly (lambda I - X): coefficient j of the product is poly[j - 1] - poly[j] X
        new = [np.zeros((N, N), dtype=np.complex128) for _ in range(len(poly) + 1)]
        for j, Pj in enumerate(poly):
            new[j + 1] += Pj
            new[j] -= Pj @ X
        poly = new
        lam_all.append(mu)
    return {"coeffs": [np.asfortranarray(c) for c in poly], "N": N, "d": d, "k": k, "lam_in": np.sort_complex(inside),
            "lam_all": np.concatenate(lam_all), "center": CENTER, "radius": RADIUS}


@functools.lru_cache(maxsize=None)
def random_coeffs(N, d, cplx, seed=20260602):
    """d + 1 Gaussian coefficient matrices scaled to unit 2-norm order (primitive-level tests: any polynomial will do)."""
    rng = np.random.default_rng([seed, N, d, int(cplx)])
    out = []
    for _ in range(d + 1):
        A = rng.standard_normal((N, N))
        if cplx:
            A = A + 1j * rng.standard_normal((N, N))
        out.append(np.asfortranarray(A / np.sqrt(N)))
    return out


def random_block(rows, cols, seed):
    rng = np.random.default_rng([seed, rows, cols])
    return np.asfortranarray(rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols)))
