"""Sparse non-normal pencils for the two-sided FEAST tests on sparse input (host only: numpy / scipy).

The matrices are grid_pencil(..., unsym=True) of tests/test_gpu_multifrontal.py: a 7-point stencil with random coefficients,
no diagonal dominance, and a tridiagonal B (or B = I).  The spectrum is scipy.linalg.eigvals of the dense copy.  The circle
comes from a rule, not from a look at what the solver finds: over the centres of the 0.1 grid in [-1, 1]^2 and k = 6 .. 12,
with d_1 <= d_2 <= ... the sorted distances of the eigenvalues from the centre, take the (centre, k) of the largest gap ratio
d_{k+1} / d_k; the radius is sqrt(d_k d_{k+1}) rounded to 3 digits, M0 = 2 k."""
import numpy as np
import scipy.linalg as sla

from test_gpu_multifrontal import grid_pencil

# (shape, seed, complex values, with B)
PARAMS = [((6, 5, 4), 1, False, False), ((10, 8, 6), 2, True, True), ((9, 8, 7), 5, False, True), ((16, 12, 1), 4, True, False)]
IDS = ["%dx%dx%d-s%d-%s-%s" % (s + (seed, "c" if cplx else "r", "B" if with_B else "I")) for (s, seed, cplx, with_B) in PARAMS]
K_RANGE = range(6, 13)
MIN_GAP_RATIO = 1.3

_cache = {}


def choose_circle(lam):
    """(centre, radius, k, gap ratio) by the rule of the module docstring; ties keep the first (centre, k) in scan order."""
    best = None
    grid = np.round(np.arange(-10, 11) * 0.1, 1)
    for re in grid:
        for im in grid:
            c = complex(re, im)
            d = np.sort(np.abs(lam - c))
            for k in K_RANGE:
                ratio = d[k] / d[k - 1]                      # d_{k+1} / d_k, 1-based
                if best is None or ratio > best[3] * (1.0 + 1e-9):      # (a real matrix: conjugate centres tie up to rounding)
                    best = (c, round(float(np.sqrt(d[k - 1] * d[k])), 3), k, float(ratio))
    return best


def make_case(shape, seed, cplx, with_B):
    """dict with A, B (scipy CSR; B None for the identity), the dense copies Ad / Bd, the spectrum lam, the circle (center,
    radius), k eigenvalues lam_in inside it (sorted by modulus, as feast_sort_general returns them), gap_ratio and M0.
    Built once per case; callers must not modify the arrays."""
    key = (shape, seed, cplx, with_B)
    if key in _cache:
        return _cache[key]
    A, B = grid_pencil(*shape, seed=seed, cplx=cplx, unsym=True)
    if not with_B:
        B = None
    Ad = A.toarray()
    Bd = None if B is None else B.toarray()
    lam = sla.eigvals(Ad) if Bd is None else sla.eigvals(Ad, Bd)
    center, radius, k, ratio = choose_circle(lam)
    inside = lam[np.abs(lam - center) < radius]
    out = {"A": A, "B": B, "Ad": Ad, "Bd": Bd, "lam": lam, "center": center, "radius": radius, "k": k, "gap_ratio": ratio,
           "lam_in": inside[np.argsort(np.abs(inside) ** 2)], "M0": 2 * k, "N": A.shape[0]}
    _cache[key] = out
    return out


_runs = {}


def reference_run(params):
    """The host restatement (tests/two_sided_reference.py, fpm[3] = 12, fpm[4] = 20) on the dense copy of a case, computed once
    and shared by the host and the GPU tests; read only."""
    from feastkit_jl_amd.parameters import feastinit
    from two_sided_reference import two_sided_reference
    if params not in _runs:
        case = make_case(*params)
        fpm = feastinit()
        fpm[3], fpm[4] = 12, 20
        _runs[params] = two_sided_reference(case["Ad"], case["Bd"], case["center"], case["radius"], case["M0"], fpm)
    return _runs[params]
