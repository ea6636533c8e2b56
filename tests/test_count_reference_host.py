"""Host checks of the eigenvalue-count estimate of feast_polynomial / feast_nonlinear (no GPU): the numpy restatement
(count_reference.py) against the spectra the case files know in closed form, the derivative tables of hip_backend, the M0 rules
and the argument errors that are raised before an engine exists.

Exact traces sum_e w_e tr(T'(z_e) T(z_e)^-1) on 16 Gauss nodes, as recorded when the estimate was designed (two decimals):
DRIVER_CASES 5.99, 5.99, 7.05, 7.05, 4.99; damped 20x16 4.98, 24x18 4.92; rational 14.31; grid delay (6,5,4) 2.13, (12,10,8) 8.83;
delay (33, 1) 5.02; the empty circle (33, 3) 0.05.  "To the digits shown" is agreement after rounding to two decimals, less than
0.005.  One recorded value does not meet that and is not the one asserted: the 24x18 trace is 4.91462 (the closed-form filter sum
over the known spectrum gives the same to 1e-9), which is 4.91 to two decimals; the recorded 4.92 is a double rounding of it
(4.9146 -> 4.915 -> 4.92).  The test asserts 4.91."""
import functools
import math

import numpy as np
import pytest

import count_reference as cr
import feastkit_jl_amd as fk
import nonlinear_cases as nc
import polynomial_cases as pc
import polynomial_sparse_cases as sc
from feastkit_jl_amd import api, hip_backend as hb
from test_estimate import rademacher

DIGITS = 0.005         # agreement after rounding to the two decimals of the recorded table


def contour(center, radius, ne=16, trapezoid=False):
    fpm = fk.feastinit()
    fpm[8] = ne
    if trapezoid:
        fpm[16] = 1
    return fk.feast_gcontour(center, radius, fk.feastdefault(fpm))


def _poly_trace(case, d):
    Z, W = contour(case["center"], case["radius"])
    return cr.exact_trace(case["coeffs"], *cr.poly_tables(d, Z, W))


def _term_trace(case):
    Z, W = contour(case["center"], case["radius"])
    return cr.exact_trace([t[0] for t in case["terms"]], *cr.term_tables([t[1] for t in case["terms"]], Z, W))


@pytest.mark.parametrize("case,recorded", list(zip(pc.DRIVER_CASES, (5.99, 5.99, 7.05, 7.05, 4.99))), ids=pc.DRIVER_IDS)
def test_trace_of_the_dense_polynomial_cases(case, recorded):
    N, d, k, _, monic = case
    c = pc.make_case(N, d, k, monic)
    tr = _poly_trace(c, d)
    print("trace %.4f%+.4fi, recorded %.2f, inside %d" % (tr.real, tr.imag, recorded, len(c["lam_in"])))
    assert abs(tr.real - recorded) < DIGITS
    assert cr.count(tr) == len(c["lam_in"]) == k


@pytest.mark.parametrize("name,recorded", [("20x16", 4.98), ("24x18", 4.91)])          # (4.91: see the module docstring)
def test_trace_of_the_damped_cases(name, recorded):
    for scaled in (False, True):          # the complex diagonal scaling leaves the spectrum, and so the trace, as it is
        c = sc.damped_case(name, scaled)
        tr = _poly_trace(c, 2)
        print("%s scaled %d: trace %.4f%+.4fi, recorded %.2f, inside %d" % (name, scaled, tr.real, tr.imag, recorded, len(c["lam_in"])))
        assert abs(tr.real - recorded) < DIGITS
        assert cr.count(tr) == len(c["lam_in"]) == c["k"]
        # the closed form: every eigenvalue contributes its filter value sum_e w_e / (z_e - lambda)
        Z, W = contour(c["center"], c["radius"])
        assert abs(tr - (W[None, :] / (Z[None, :] - c["lam_all"][:, None])).sum()) <= 1e-9


NONLINEAR = [("rational", lambda: nc.rational_case(), 14.31), ("grid-6x5x4", lambda: nc.grid_delay_case((6, 5, 4)), 2.13),
             ("grid-12x10x8", lambda: nc.grid_delay_case((12, 10, 8)), 8.83), ("delay-33-1", lambda: nc.delay_case(33, 1), 5.02),
             ("delay-33-3-empty", lambda: nc.delay_case(33, 3), 0.05)]


@pytest.mark.parametrize("make,recorded", [(m, r) for _, m, r in NONLINEAR], ids=[n for n, _, _ in NONLINEAR])
def test_trace_of_the_nonlinear_cases(make, recorded):
    c = make()
    tr = _term_trace(c)
    print("trace %.4f%+.4fi, recorded %.2f, inside %d" % (tr.real, tr.imag, recorded, c["count"]))
    assert abs(tr.real - recorded) < DIGITS
    assert cr.count(tr) == c["count"]


@functools.lru_cache(maxsize=None)
def _damped_samples():
    c = sc.damped_case("20x16", False)
    Z, W = contour(c["center"], c["radius"])
    F, G = cr.poly_tables(2, Z, W)
    V = np.concatenate([rademacher(seed, np.arange(c["N"]), np.arange(64)) for seed in range(1, 8)], axis=1)
    t, _ = cr.samples(c["coeffs"], F, G, V)
    return t.reshape(7, 64)


def test_hutchinson_mean_is_unbiased_over_seeds():
    """64 Rademacher columns per seed, seeds 1 .. 7: the mean of all of them within 4 standard errors of the exact trace 4.98,
    and the standard error of one seed in the range recorded for these cases (0.3 .. 0.6)"""
    t = _damped_samples()
    mean, stderr = cr.mean_stderr(t.ravel())
    per_seed = [cr.mean_stderr(row) for row in t]
    print("pooled mean %.3f%+.3fi stderr %.3f; per seed %s" % (mean.real, mean.imag, stderr, ["%.2f +- %.2f" % (m.real, s) for m, s in per_seed]))
    assert abs(mean.real - 4.98) <= 4.0 * stderr
    assert all(0.2 <= s <= 0.7 for _, s in per_seed)


def test_derivative_tables():
    Z, _ = contour(-0.4 + 0.3j, 1.3)
    tau, s = 0.8, 2.5 - 0.7j
    funcs = hb.nep_functions([0, 1, 3, lambda z: np.exp(-tau * z), lambda z: 1.0 / (z - s)])
    D = hb.nep_derivative_table(funcs, Z)
    exact = np.stack([np.zeros_like(Z), np.ones_like(Z), 3.0 * Z ** 2, -tau * np.exp(-tau * Z), -1.0 / (Z - s) ** 2], axis=1)
    assert D.shape == exact.shape == (16, 5)
    assert np.all(D[:, 0] == 0.0)                      # a constant term drops out exactly
    rel = np.abs(D[:, 1:] - exact[:, 1:]) / np.abs(exact[:, 1:])
    print("largest relative error of the central differences: %.2e" % rel.max())
    assert rel.max() <= 1e-8
    # the restatement forms the same quantity
    _, G = cr.term_tables(funcs, Z, np.ones(16))
    assert np.abs(G - D).max() <= 1e-12 * np.abs(D).max()
    # a polynomial: exact, column 0 zero
    P = hb.poly_derivative_table(3, Z)
    assert np.array_equal(P[:, 0], np.zeros(16)) and np.allclose(P[:, 3], 3.0 * Z ** 2, rtol=1e-15, atol=0.0)
    assert np.abs(cr.poly_tables(3, Z, np.ones(16))[1] - P).max() <= 1e-15 * np.abs(P).max()


def test_derivative_table_refuses_a_pole_next_to_a_node():
    Z, _ = contour(0.0, 1.0)
    h = hb.NEWTON_FD * max(1.0, abs(Z[2]))
    with pytest.raises(ValueError, match="f_1 is not finite"):
        with np.errstate(all="ignore"):
            hb.nep_derivative_table(hb.nep_functions([1, lambda z: 1.0 / (z - (Z[2] + h))]), Z)


def test_M0_rules():
    for mean, stderr, N, d, want, want_lin in ((4.98 - 0.04j, 0.45, 320, 2, 9, 5), (0.05, 0.2, 33, 1, 8, 8), (14.31, 0.5, 40, 3, 23, 8),
                                               (40.0, 1.0, 45, 8, 45, 6), (2.13, 0.0, 6, 2, 6, 3)):
        est = {"mean": complex(mean), "stderr": stderr}
        assert cr.auto_M0(mean, stderr, N) == api.auto_M0(est, N) == want
        assert cr.auto_M0_linearised(mean, stderr, N, d) == max(1, math.ceil(want / d)) == want_lin
    assert cr.count(4.6 + 3j) == 5 and cr.count(-0.7) == 0


def test_argument_errors_before_any_engine():
    c = pc.make_case(70, 2, 6, True)
    terms = nc.rational_case()["terms"]
    Q0 = np.zeros((70, 4))
    with pytest.raises(ValueError, match="M0 must be an integer or 'auto'"):
        fk.feast_polynomial(c["coeffs"], c["center"], c["radius"], M0="automatic")
    with pytest.raises(ValueError, match="M0 must be an integer or 'auto'"):
        fk.feast_nonlinear(terms, 0.5, 0.6, M0="Auto")
    with pytest.raises(ValueError, match="Q0"):
        fk.feast_polynomial(c["coeffs"], c["center"], c["radius"], M0="auto", Q0=Q0)
    with pytest.raises(ValueError, match="Q0"):
        fk.feast_nonlinear(terms, 0.5, 0.6, M0="auto", Q0=Q0)
    fpm = fk.feastinit()
    fpm[14] = 2
    with pytest.raises(ValueError, match="sample count"):
        fk.feast_polynomial(c["coeffs"], c["center"], c["radius"], M0="auto", fpm=fpm.copy())
    with pytest.raises(ValueError, match="sample count"):
        fk.feast_nonlinear(terms, 0.5, 0.6, M0="auto", fpm=fpm.copy())
    # the arguments the estimate does not use are still validated
    with pytest.raises(ValueError, match="method"):
        fk.feast_polynomial(c["coeffs"], c["center"], c["radius"], M0=8, fpm=fpm.copy(), method="subspace")
    with pytest.raises(ValueError, match="moments"):
        fk.feast_nonlinear(terms, 0.5, 0.6, M0=8, fpm=fpm.copy(), moments=0)
    # feastdefault gives the estimate its own node count when the caller left fpm[8] unset
    assert int(fk.feastdefault(fpm.copy())[8]) == 6
