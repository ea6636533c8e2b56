"""feast_polynomial, the host half: the cases of tests/polynomial_cases.py have the spectrum they were built for, the
structured shifted solve of tests/polynomial_reference.py equals the dense companion solve, the restatement's driver agrees
with the oracle's feast_general on the explicit companion pencil, and the keyword validation of feast_polynomial touches no
device."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import feast_oracle as fo
import feastkit_jl_amd as fk
import polynomial_cases as pc
import polynomial_reference as pr


@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_cases_have_k_eigenvalues_inside(params):
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    A, B = pr.companion(case["coeffs"])
    lam = sla.eigvals(A, B)
    dist = np.abs(lam - case["center"])
    inside = lam[dist <= case["radius"]]
    print("inside %d, nearest outside at %.3f r, farthest inside at %.3f r" % (
        len(inside), dist[dist > case["radius"]].min() / case["radius"], dist[dist <= case["radius"]].max() / case["radius"]))
    assert len(inside) == k
    assert pr.match_error(inside, case["lam_in"]) <= 1e-9
    assert M0 * d >= k


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_structured_solve_equals_companion_solve(d):
    N, m = 23, 5
    coeffs = pc.random_coeffs(N, d, True)
    A, B = pr.companion(coeffs)
    R = pc.random_block(d * N, m, 7)
    for z in (0.3 + 1.2j, -0.7 + 0.2j):
        ref = np.linalg.solve(z * B - A, R)
        got = pr.structured_solve(coeffs, z, R)
        err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print("d %d z %s relative difference %.2e" % (d, z, err))
        assert err <= 1e-12


@pytest.mark.parametrize("params", [p for p in pc.DRIVER_CASES if p[4]], ids=[i for p, i in zip(pc.DRIVER_CASES, pc.DRIVER_IDS) if p[4]])
def test_restatement_agrees_with_the_oracle_on_the_companion(params):
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    A, B = pr.companion(case["coeffs"])
    Q0 = fo.seeded_subspace(d * N, M0 * d, 20260515)
    ours = pr.driver(case["coeffs"], case["center"], case["radius"], M0, Q0=Q0, residual="reference")
    ref = fo.feast_general(A, B, case["center"], case["radius"], M0 * d, ne=pc.NE, fpm3=pc.FPM3, Q0=Q0)
    print("restatement loop %d epsout %.2e | oracle loop %d epsout %.2e" % (ours["loop"], ours["epsout"], ref.loop, ref.epsout))
    assert ours["info"] == ref.info == 0
    assert ours["M"] == ref.M == k
    assert abs(ours["loop"] - ref.loop) <= 1
    assert pr.match_error(ours["lam"], ref.lam) <= 1e-9


@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_restatement_converges_with_the_pencil_residual(params):
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    run = pr.driver_run(params)
    print("loop %d epsout %.2e history %s eigenvalue error %.2e backward error %.2e" % (
        run["loop"], run["epsout"], ["%.1e" % e for e in run["eps_hist"]], pr.match_error(run["lam"], case["lam_in"]),
        run["backward_error"].max()))
    assert run["info"] == 0 and run["M"] == k
    assert run["epsout"] <= 1e-10
    # the stop must not hang on rounding: the loop before the last is clear of the threshold as well
    assert len(run["eps_hist"]) == 1 or run["eps_hist"][-2] > 3e-10
    assert run["epsout"] < 1e-10 / 3
    assert pr.match_error(run["lam"], case["lam_in"]) <= 1e-9
    assert run["backward_error"].max() <= 1e-11


def _coeffs(n=6, count=3):
    rng = np.random.default_rng(5)
    return [rng.standard_normal((n, n)) for _ in range(count)]


@pytest.mark.parametrize("args,kw,word", [
    (([np.eye(4)], 0.0, 1.0), {}, "at least two"),
    ((_coeffs(4, 10), 0.0, 1.0), {}, "degree"),
    (([np.eye(4), np.ones((4, 5))], 0.0, 1.0), {}, "square"),
    (([np.eye(4), np.eye(5)], 0.0, 1.0), {}, "equal shapes"),
    ((_coeffs(), 0.0, 0.0), {}, "radius"),
    ((_coeffs(), 0.0, -1.0), {}, "radius"),
    ((_coeffs(), 0.0, 1.0), {"residual": "relative"}, "residual"),
])
def test_keyword_validation_is_host_only(args, kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    with pytest.raises(ValueError, match=word):
        fk.feast_polynomial(*args, M0=3, **kw)


def test_sparse_coefficients_beyond_the_dense_window_are_refused(monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    n = fk.api.POLY_DENSE_LIMIT + 1
    I = sp.identity(n, format="csr")
    with pytest.raises(ValueError, match="sparse"):
        fk.feast_polynomial([I, I, I], 0.0, 1.0, M0=3)


def test_valid_input_reaches_the_engine_and_feast_pep_is_the_same_entry(monkeypatch):
    class Reached(Exception):
        pass

    def no_engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(fk.api, "_engine", no_engine)
    assert fk.feast_pep is fk.feast_polynomial
    with pytest.raises(Reached):
        fk.feast_polynomial(_coeffs(), 0.0, 1.0, M0=3)
    with pytest.raises(Reached):
        fk.feast_polynomial([sp.csr_matrix(c) for c in _coeffs()], 0.0, 1.0, M0=3, residual="reference")


def test_symbols_are_declared():
    for name in ("feasthip_set_polynomial", "feasthip_poly_solve_dev", "feasthip_poly_contour_apply_dev", "feasthip_poly_matmul_dev",
                 "feasthip_poly_project_dev", "feasthip_poly_ritz_residual_dev"):
        assert name in fk.SYMBOLS
