"""Panels for the rank-revealing Cholesky-QR tests: X = U diag(s) W^H with random orthonormal U, W, generated from a seed.
Every case states its own precondition from scipy's column-pivoted QR alone (assert_unambiguous): no |R_ii| / |R_11| within
a factor 30 of the rank threshold in use, so the reference's rank is not a matter of rounding.

A panel graded geometrically from 1 to 1e-14 ("c") always has singular values next to the threshold sqrt(eps); the
precondition cannot hold for it under any seed.  Case c therefore leaves out the values within a factor 1e3 of the
threshold and keeps the grading on both sides, which still spans more than one stage above the threshold."""
import numpy as np
import scipy.linalg as sla

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))
EPS = float(np.finfo(np.float64).eps)
MARGIN = 30.0


def _orth(rng, n, k, cplx):
    A = rng.standard_normal((n, k))
    if cplx:
        A = A + 1j * rng.standard_normal((n, k))
    return np.linalg.qr(A)[0]


def _panel(rng, N, m, s, cplx):
    X = (_orth(rng, N, m, cplx) * s) @ _orth(rng, m, m, cplx).conj().T
    return X.astype(complex)


def make_case(kind, N, m, cplx, seed):
    """-> (X, ref_scale).  kind: a full rank | b gap | c graded | d duplicates and zero columns | e_small, e_big scaled by
    1e-150 / 1e+150 | f block of a wider matrix (ref_scale 1e5 times its own largest norm) | zero."""
    rng = np.random.default_rng(seed)
    ref = 0.0
    if kind == "a":
        X = _panel(rng, N, m, np.linspace(1.0, 2.0, m), cplx)
    elif kind in ("b", "e_small", "e_big", "f"):
        r = max(1, (2 * m) // 3)
        s = np.concatenate([np.geomspace(1.0, 1e-5, r) if r > 1 else np.ones(1),
                            np.geomspace(1e-11, 1e-14, m - r) if m - r > 1 else 1e-12 * np.ones(m - r)])
        if kind == "f":      # the wider matrix has columns 1e5 times longer: full rank on its own, not as a block of it
            s = np.concatenate([np.geomspace(1.0, 0.1, r) if r > 1 else np.ones(1),
                                np.geomspace(5e-6, 2e-6, m - r) if m - r > 1 else 5e-6 * np.ones(m - r)])
        X = _panel(rng, N, m, s, cplx)
        if kind == "e_small":
            X = X * 1e-150
        if kind == "e_big":
            X = X * 1e+150
        if kind == "f":
            ref = 1e5 * np.linalg.norm(X, axis=0).max()
    elif kind == "c":
        s = np.geomspace(1.0, 1e-14, m) if m > 1 else np.ones(1)
        keep = (s > 1e3 * SQRT_EPS) | (s < SQRT_EPS / 1e3)
        s = np.concatenate([s[keep], np.geomspace(1e-12, 1e-14, m - keep.sum())]) if m - keep.sum() else s
        X = _panel(rng, N, m, s, cplx)
    elif kind == "d":
        r = max(1, m // 2)
        B = _panel(rng, N, r, np.linspace(1.0, 2.0, r), cplx)
        X = np.zeros((N, m), dtype=complex)
        for j in range(m):
            if j % 5 == 4 and m > 4:
                continue                       # zero column
            X[:, j] = B[:, j % r]              # exact duplicates from column r on
    elif kind == "zero":
        X = np.zeros((N, m), dtype=complex)
    else:
        raise ValueError(kind)
    return X, float(ref)


def threshold(rank_tol, N, m, big_dim=0):
    return max(rank_tol, EPS * max(N, big_dim, m))


def scipy_qr(X, rank_tol, ref_scale=0.0, big_dim=0):
    """scipy's column-pivoted QR and the reference's rank rule -> (rank, perm, |R_ii|, R_11 in use, threshold)."""
    N, m = X.shape
    _, R, piv = sla.qr(X, mode="economic", pivoting=True)
    rd = np.abs(np.diag(R))
    r11 = max(rd[0] if rd.size else 0.0, ref_scale)
    thr = threshold(rank_tol, N, m, big_dim)
    rank = 0
    while rank < m and rd[rank] > thr * r11 and rd[rank] > 0:
        rank += 1
    return rank, piv, rd, r11, thr


def assert_unambiguous(X, rank_tol, ref_scale=0.0, big_dim=0):
    rank, piv, rd, r11, thr = scipy_qr(X, rank_tol, ref_scale, big_dim)
    if r11 > 0:
        rel = rd / r11
        near = (rel > thr / MARGIN) & (rel < thr * MARGIN)
        assert not near.any(), ("|R_ii|/|R_11| within a factor 30 of the threshold", rel[near], thr)
    return rank, piv, rd, r11, thr


KINDS = ("a", "b", "c", "d", "e_small", "e_big", "f")
