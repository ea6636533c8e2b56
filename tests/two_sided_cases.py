"""Pencils with a prescribed spectrum for the two-sided FEAST tests (host only, numpy).

    A = X Lambda X^-1,  X = I + c G / sqrt(N)            (non-normal: cond(X) grows with c)
    optionally  B = I + 0.3 G' / sqrt(N)  general complex,  A <- B A     (A x = lambda B x keeps X and Lambda)

n_in eigenvalues lie inside radius 0.7 (a sunflower spiral, so their moduli are distinct and their mutual gaps are known),
the other N - n_in at modulus >= 1.3; the contour is the unit circle."""
import numpy as np

CASES = [(96, 12, 7, 0.3), (130, 16, 9, 0.6), (257, 24, 14, 0.45), (384, 32, 20, 0.6)]      # (N, M0, n_in, c)
PARAMS = [(N, M0, n_in, c, with_B) for (N, M0, n_in, c) in CASES for with_B in (False, True)]
IDS = ["N%d-M0_%d-%s" % (N, M0, "B" if with_B else "I") for (N, M0, _, _, with_B) in PARAMS]
CENTER, RADIUS = 0.0, 1.0

_cache = {}


def make_case(N, M0, n_in, c, with_B):
    """dict with A, B (None or complex), lam_in (sorted by modulus, as feast_sort_general returns them), gap (smallest distance
    between two inside eigenvalues), X_in / Y_in (exact right / left eigenvectors of lam_in, unit columns) and overlap
    (|y_j^H B x_j| of those unit vectors).  Built once per case; callers must not modify the arrays."""
    key = (N, M0, n_in, c, with_B)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([N, M0, n_in, int(1000 * c), int(with_B)])
    k = np.arange(n_in)
    lam_in = 0.7 * np.sqrt((k + 0.5) / n_in) * np.exp(1j * k * np.pi * (3.0 - np.sqrt(5.0)))
    n_out = N - n_in
    lam_out = (1.3 + 1.7 * rng.random(n_out)) * np.exp(2j * np.pi * rng.random(n_out))
    lam = np.concatenate([lam_in, lam_out])
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    X = np.eye(N) + c * G / np.sqrt(N)
    Xinv = np.linalg.inv(X)
    A = (X * lam[None, :]) @ Xinv
    B = None
    if with_B:
        G2 = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        B = np.eye(N) + 0.3 * G2 / np.sqrt(N)
        A = B @ A
    # left eigenvectors: y^H A = lambda y^H B  <=>  y^H B = row of X^-1
    Yh = Xinv[:n_in, :] if B is None else np.linalg.solve(B.T, Xinv[:n_in, :].T).T
    X_in = X[:, :n_in] / np.linalg.norm(X[:, :n_in], axis=0)
    Y_in = Yh.conj().T
    Y_in = Y_in / np.linalg.norm(Y_in, axis=0)
    BX = X_in if B is None else B @ X_in
    overlap = np.abs(np.einsum("ij,ij->j", Y_in.conj(), BX))
    d = np.abs(lam_in[:, None] - lam_in[None, :]) + np.diag(np.full(n_in, np.inf))
    out = {"N": N, "M0": M0, "n_in": n_in, "A": np.asfortranarray(A), "B": None if B is None else np.asfortranarray(B),
           "lam_in": lam_in, "gap": float(d.min()), "X_in": X_in, "Y_in": Y_in, "overlap": overlap,
           "cond_X": float(np.linalg.cond(X))}
    _cache[key] = out
    return out
