"""The numpy restatement of feast_nonlinear (tests/nonlinear_reference.py) on the closed-form cases of tests/nonlinear_cases.py:
it finds exactly the eigenvalues inside every circle from three start seeds, returns nothing for the empty circle, loses
eigenvalues with one Beyn moment where eigenvalues share an eigenvector (the rule that matters, pinned), and reproduces the
polynomial restatement on a polynomial posed as terms.  No GPU: this is what tests/test_gpu_nonlinear.py holds the device to."""
import numpy as np
import pytest

import nonlinear_cases as nc
import nonlinear_reference as nr
import polynomial_cases as pc
import polynomial_projected_reference as ppr

# both restatements stop at a backward error of 1e-10, so their eigenvalues agree to the accuracy either reaches: measured on the
# three cases below with start seed 1: 2.9e-14, 1.1e-11, 9.4e-11.  The bound is ten times the largest.
POLY_AGREEMENT = 10 * 9.4e-11
POLY_CASES = pc.DRIVER_CASES[:3]


def _check(out, case):
    err = nr.match_error(out["lam"], case["lam_in"]) if out["M"] == case["count"] else np.inf
    print("count %d M %d loop %d history %s rank %s candidates %s eigenvalue error %.2e" % (
        case["count"], out["M"], out["loop"], ["%.1e" % e for e in out["eps_history"]], out["rank"], out["candidates"], err))
    assert out["info"] == 0 and out["M"] == case["count"]
    assert out["epsout"] <= 1e-10 and err <= 1e-7
    assert np.abs(np.linalg.norm(out["q"], axis=0) - 1.0).max() <= 1e-12


def test_closed_forms_satisfy_their_equations():
    """the Lambert roots solve the scalar equations, and T(lambda) is singular there"""
    case = nc.delay_case(33, 0)
    mats, funcs = nr.split(case["terms"])
    for lam in case["lam_in"]:
        s = np.linalg.svd(nr.t_at(mats, nr.table(funcs, lam)[0]), compute_uv=False)
        assert s[-1] <= 1e-10 * s[0]
    grid = nc.grid_delay_case((6, 5, 4))
    mats, funcs = nr.split(grid["terms"])
    for lam in grid["lam_in"]:
        s = np.linalg.svd(nr.t_at(mats, nr.table(funcs, lam)[0]), compute_uv=False)
        assert s[-1] <= 1e-10 * s[0]
    assert nc.delay_case(*nc.EMPTY_CASE)["count"] == 0
    assert all(nc.delay_case(N, c)["count"] > 0 for N, c in nc.DELAY_CASES)
    assert any(nc.shared_vector_count(nc.delay_case(N, c)) for N, c in nc.DELAY_CASES)


@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("N,circle", nc.DELAY_CASES, ids=nc.DELAY_IDS)
def test_delay_cases(N, circle, seed):
    _check(nr.delay_run(N, circle, seed), nc.delay_case(N, circle))


@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("dims", list(nc.GRID_CASES), ids=nc.GRID_IDS)
def test_grid_delay_cases(dims, seed):
    _check(nr.grid_run(dims, False, seed), nc.grid_delay_case(dims))


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_rational_case(seed):
    _check(nr.rational_run(seed), nc.rational_case())


@pytest.mark.parametrize("seed", nc.SEEDS)
def test_empty_circle(seed):
    out = nr.delay_run(*nc.EMPTY_CASE, seed)
    assert out["M"] == 0 and out["info"] == 2 and len(out["lam"]) == 0 and out["candidates"][-1] == 0


@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("N,circle", [nc_ for nc_ in nc.DELAY_CASES if nc.shared_vector_count(nc.delay_case(*nc_))])
def test_one_moment_loses_eigenvalues_that_share_a_vector(N, circle, seed):
    case = nc.delay_case(N, circle)
    one = nr.delay_run(N, circle, seed, moments=1)
    two = nr.delay_run(N, circle, seed)
    print("count %d (%d share a vector): one moment M %d, two moments M %d" % (case["count"], nc.shared_vector_count(case), one["M"], two["M"]))
    assert two["M"] == case["count"] and one["M"] < case["count"]


@pytest.mark.parametrize("params", POLY_CASES, ids=pc.DRIVER_IDS[:3])
def test_polynomial_posed_as_terms(params):
    N, d, k, _, monic = params
    case = nc.poly_as_terms(pc.make_case(N, d, k, monic))
    out = nr.driver(case["terms"], case["center"], case["radius"], k + 2, seed=1)
    ref = ppr.dense_run((N, d, k, monic), k + 2, 1)
    diff = nr.match_error(out["lam"], ref["lam"]) if out["M"] == ref["M"] else np.inf
    print("M %d loop %d (polynomial restatement: M %d loop %d), eigenvalue difference %.2e" % (out["M"], out["loop"], ref["M"], ref["loop"], diff))
    assert out["info"] == ref["info"] == 0 and out["M"] == ref["M"] == k
    assert diff <= POLY_AGREEMENT
