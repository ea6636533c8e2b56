"""feast_nonlinear without a GPU: every argument check (all of them run before an engine is made), the new entry points in the
built library, the table helpers and the two host rules of the reduced solve (hip_backend.nep_beyn / nep_newton_polish) against
the restatement of tests/nonlinear_reference.py."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import nonlinear_cases as nc
import nonlinear_reference as nr
from feastkit_jl_amd import _lib, hip_backend as hb

NEW_SYMBOLS = ("feasthip_set_terms", "feasthip_set_terms_csr", "feasthip_nep_set_node_values", "feasthip_nep_solve_dev",
               "feasthip_nep_eval_cols_dev", "feasthip_nep_resinv_apply_dev", "feasthip_nep_ritz_eval_dev")


class _NoEngine:
    """stands where the engine goes: a check that lets a bad argument through would touch it"""
    def __getattr__(self, name):
        raise AssertionError("the argument checks must run before the engine is used")


def _terms(N=12, sparse=False):
    I = sp.identity(N, format="csr") if sparse else np.eye(N)
    A = sp.diags(np.arange(1.0, N + 1)).tocsr() if sparse else np.diag(np.arange(1.0, N + 1))
    return [(A, 0), (I, lambda z: -z), (I, nc.exp_term(1.0))]


def test_symbols_are_declared_and_exported():
    lib = fk.load_library()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert fk.feast_nep is fk.feast_nonlinear and callable(fk.feast_hip_nonlinear)


def test_null_handles_are_refused():
    lib = fk.load_library()
    assert lib.feasthip_set_terms(None, 4, 2, 0, None, None) == 7
    assert lib.feasthip_set_terms_csr(None, 4, 2, 0, None, None, None) == 7
    assert lib.feasthip_nep_set_node_values(None, 1, None) == 7
    assert lib.feasthip_nep_solve_dev(None, 0, 1, None, None, None) == 7
    assert lib.feasthip_nep_eval_cols_dev(None, 1, None, None, None) == 7
    assert lib.feasthip_nep_resinv_apply_dev(None, 1, None, None, None, None, None, None) == 7
    assert lib.feasthip_nep_ritz_eval_dev(None, 1, None, 1, None, None, None, None) == 7


@pytest.mark.parametrize("make,match", [
    (lambda: dict(terms=_terms()[:1]), "2 to 9 terms"),
    (lambda: dict(terms=_terms() * 4), "2 to 9 terms"),
    (lambda: dict(terms=[(np.eye(12),)] * 2), "pair"),
    (lambda: dict(terms=[(np.ones((12, 11)), 0), (np.eye(12), 1)]), "square"),
    (lambda: dict(terms=[(np.eye(11), 0), (np.eye(12), 1)]), "equal shapes"),
    (lambda: dict(terms=[(np.eye(12), 0), (sp.identity(12, format="csr"), 1)], solver="sparse_direct"), "no mix"),
    (lambda: dict(terms=_terms(), solver="sparse_direct"), "scipy.sparse"),
    (lambda: dict(terms=_terms(), radius=0.0), "radius"),
    (lambda: dict(terms=_terms(), radius=-1.0), "radius"),
    (lambda: dict(terms=_terms(), Q0=np.ones((12, 3))), "Q0"),
    (lambda: dict(terms=_terms(), moments=0), "moments"),
    (lambda: dict(terms=_terms(), reduced_nodes=7), "reduced_nodes"),
    (lambda: dict(terms=_terms(sparse=True), solver="bicgstab"), "out of scope"),
    (lambda: dict(terms=_terms(sparse=True), solver="cocg"), "out of scope"),
    (lambda: dict(terms=_terms(sparse=True), solver="gmres"), "out of scope"),
    (lambda: dict(terms=_terms(), solver="banded"), "solver must be"),
    (lambda: dict(terms=_terms(), ortho="householder"), "ortho"),
    (lambda: dict(terms=[(np.eye(12), 0), (np.eye(12), -1)]), "non-negative int"),
    (lambda: dict(terms=[(np.eye(12), 0), (np.eye(12), "exp")]), "callable"),
    (lambda: dict(terms=[(np.eye(12), 0), (np.eye(12), lambda z: 1.0 / (z - z))]), "not finite at a contour node"),
    (lambda: dict(terms=[(np.eye(12), 0), (np.eye(12), lambda z: np.ones(3))]), "same shape"),
])
def test_value_errors(make, match):
    kw = dict(center=0.5, radius=1.0, M0=4, engine=_NoEngine())
    kw.update(make())
    terms = kw.pop("terms")
    center, radius = kw.pop("center"), kw.pop("radius")
    with pytest.raises(ValueError, match=match):
        fk.feast_nonlinear(terms, center, radius, **kw)


def test_a_pole_on_a_node_names_the_function():
    fpm = fk.feastinit()
    fpm[8] = 16
    fk.feastdefault(fpm)
    z0 = fk.feast_gcontour(0.5 + 0j, 1.0, fpm)[0][3]
    with pytest.raises(ValueError, match="f_2 is not finite"):
        fk.feast_nonlinear([(np.eye(6), 0), (np.eye(6), 1), (np.eye(6), lambda z: 1.0 / (z - z0))], 0.5, 1.0, fpm=fpm, engine=_NoEngine())


def test_table_helpers():
    funcs = hb.nep_functions([0, 3, nc.exp_term(0.5), lambda z: 2.0 + 0j])
    z = np.array([0.3 - 0.2j, 1.5j, -2.0])
    F = hb.nep_table(funcs, z)
    assert F.shape == (3, 4) and F.dtype == np.complex128
    assert np.array_equal(F[:, 0], np.ones(3)) and np.allclose(F[:, 1], z ** 3, rtol=1e-15)
    assert np.allclose(F[:, 2], np.exp(-0.5 * z), rtol=1e-15) and np.array_equal(F[:, 3], np.full(3, 2.0))       # a scalar is broadcast
    assert hb.nep_table(funcs, 0.7).shape == (1, 4)
    assert np.array_equal(F, nr.table([nr.as_function(f) for f in (0, 3, nc.exp_term(0.5), lambda z: 2.0 + 0j)], z))
    with pytest.raises(ValueError):
        hb.nep_functions([True])
    # a pole gives a non-finite entry and no warning or exception: the callers decide
    G = hb.nep_table([lambda z: 1.0 / z], np.array([0.0, 1.0]))
    assert not np.isfinite(G[0, 0]) and G[1, 0] == 1.0


def test_reduced_solve_matches_the_restatement_and_the_closed_form():
    """the package's Beyn and Newton steps on a small delay problem taken whole (Q = I): the eigenvalues inside, the shared
    vectors included, to the accuracy of the polish, and the same numbers as the restatement's"""
    case = nc.delay_case(33, 2)
    mats, funcs = nr.split(case["terms"])
    c, rho = case["center"], case["radius"]
    theta, Y = hb.nep_beyn(mats, funcs, c, rho, 2, 128)
    theta_r, Y_r = nr.beyn(mats, funcs, c, rho, 2, 128)
    assert len(theta) == len(theta_r) and nr.match_error(theta, theta_r) <= 1e-9
    pol = np.array([hb.nep_newton_polish(mats, funcs, theta[i], Y[:, i], rho)[0] for i in range(len(theta))])
    inside = pol[np.abs(pol - c) <= rho]
    print("Beyn candidates %d, inside after the polish %d of %d" % (len(theta), len(inside), case["count"]))
    assert len(inside) == case["count"] and nr.match_error(inside, case["lam_in"]) <= 1e-11
    assert nc.shared_vector_count(case) > 0
    one, _ = hb.nep_beyn(mats, funcs, c, rho, 1, 128)
    assert np.sum(np.abs(one - c) <= rho) <= 33          # (one moment: at most r candidates)
    # an empty circle returns nothing
    empty = nc.delay_case(*nc.EMPTY_CASE)
    mats, funcs = nr.split(empty["terms"])
    assert len(hb.nep_beyn(mats, funcs, empty["center"], empty["radius"], 2, 128)[0]) == 0


def test_newton_guard_keeps_the_start_pair():
    """a start far from any root: the polished value is rejected (it moves further than NEWTON_REACH radius, or does not
    reduce the residual) and the start pair comes back with a unit vector"""
    case = nc.delay_case(33, 1)
    mats, funcs = nr.split(case["terms"])
    rng = np.random.default_rng(5)
    v = rng.standard_normal(33) + 1j * rng.standard_normal(33)
    far = case["center"] + 40.0j
    th, w = hb.nep_newton_polish(mats, funcs, far, v, 1e-3)
    assert th == far and abs(np.linalg.norm(w) - 1.0) <= 1e-14
    th_r, _ = nr.newton_polish(mats, funcs, far, v, 1e-3)
    assert th_r == far
    # and a start next to a root converges to it
    lam = case["lam_in"][0]
    i = int(np.argmin(np.min(np.abs(case["roots"] - lam), axis=1)))
    th, w = hb.nep_newton_polish(mats, funcs, lam + 1e-4, case["V"][:, i] + 1e-4 * v, case["radius"])
    assert abs(th - lam) <= 1e-12
    assert (hb.BEYN_RANK_TOL, hb.NEWTON_STEPS, hb.NEWTON_FD, hb.NEWTON_DONE, hb.NEWTON_REACH) == (1e-10, 6, 1e-6, 1e-14, 0.1)
