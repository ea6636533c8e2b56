"""Krylov solves on P(z) for sparse coefficients, the host half: the restatement of the operator (polynomial_krylov_reference.PolyOp)
against plain linear algebra, the pinned inexact runs of the projected driver, the conditions on the reference alone that the
device comparison of test_gpu_polynomial_krylov.py rests on, and the keyword validation, which touches no device."""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import gmres_reference as gr
import krylov_reference as kr
import polynomial_krylov_reference as pk
import polynomial_projected_reference as ppr
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from test_gpu_primitives import rand_block
from test_polynomial_projected_host import _clears

EPS = np.finfo(np.float64).eps
OPERATORS = [("mixed",) + m for m in pk.MIXED] + [("damped", 0), ("damped", 5)]


# ---- the restatement against plain linear algebra ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", OPERATORS, ids=pk.case_id)
def test_polyop_is_the_dense_product(key):
    coeffs, z = pk._operator(key)
    N = coeffs[0].shape[0]
    x = rand_block(N, 1, 5)[:, 0]
    want = pk.dense_poly(coeffs, z) @ x.astype(np.clongdouble)
    got = pk.PolyOp(coeffs, np.clongdouble).apply(z, x)
    leps = np.finfo(np.longdouble).eps
    assert kr.rel_dist(got, want) <= 64 * leps
    got64 = pk.PolyOp(coeffs, np.complex128).apply(z, x)
    assert got64.dtype == np.complex128 and kr.rel_dist(got64, want) <= 64 * EPS


@pytest.mark.parametrize("key,method", [(("mixed", sc.GRIDS[0], 3, True), "bicgstab"), (("damped", 5), "cocg5"), (("damped", 5), "bicgstab")],
                         ids=["mixed-bicgstab", "damped-cocg", "damped-bicgstab"])
def test_reference_solves_solve(key, method):
    """rtol = 1e-13 in long double: the iterate is numpy.linalg.solve's to the conditioning of P(z)"""
    coeffs, z = pk._operator(key)
    N = coeffs[0].shape[0]
    b = rand_block(N, 1, 6)[:, 0]
    P = pk.dense_poly(coeffs, z, np.complex128)
    want = np.linalg.solve(P, b)
    col = kr.solve_column(pk.PolyOp(coeffs, np.clongdouble), z, b, method, 1e-13, 0.0, 2000)
    assert col.status == 0 and not col.active
    assert kr.rel_dist(col.x, want) <= 10 * np.linalg.cond(P) * 1e-13


def test_reference_gmres_solves():
    coeffs, z = pk._operator(pk.GMRES_KEY)
    N = coeffs[0].shape[0]
    B = rand_block(N, 3, 7)
    P = pk.dense_poly(coeffs, z, np.complex128)
    want = np.linalg.solve(P, B)
    batch = gr.solve_batch(pk.PolyOp(coeffs, np.clongdouble), [z], B, None, 1e-13, 0.0, 2000, 30)
    for j, col in enumerate(batch.cols[0]):
        assert col.status == 0 and not col.active
        assert kr.rel_dist(col.x, want[:, j]) <= 10 * np.linalg.cond(P) * 1e-13


# ---- the pinned inexact runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scaled,method,solver,rtol", pk.INEXACT_PINS, ids=pk.INEXACT_IDS)
def test_inexact_restatement_on_the_damped_cases(name, scaled, method, solver, rtol):
    """Inexact solves at solver_tol = 1e-4 keep the exact-solve loop count and history (measured: <= 4 % apart), no node
    stops at the 2000-step cap, and the count survives a 1e-14 perturbation of the start block."""
    columns, seed, loop = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    exact = ppr.damped_run(name, scaled, columns, seed)
    out = pk.inexact_run(name, scaled, method, rtol)
    err = pr.match_error(out["lam"], case["lam_in"])
    print("loop %d history %s exact %s worst column steps %s eigenvalue error %.2e" % (
        out["loop"], ["%.1e" % e for e in out["eps_history"]], ["%.1e" % e for e in exact["eps_history"]],
        [k["iterations"] for k in out["krylov"]], err))
    assert out["info"] == 0 and out["M"] == case["k"] and err <= 1e-8
    assert out["loop"] == loop == exact["loop"] and _clears(out["eps_history"], sc.FPM3)
    for a, b in zip(out["eps_history"], exact["eps_history"]):
        assert b / pk.HISTORY_FACTOR <= a <= b * pk.HISTORY_FACTOR
    assert len(out["krylov"]) == loop + 1 and not any(k["capped_nodes"] for k in out["krylov"])
    pert = pk.inexact_run(name, scaled, method, rtol, 1e-14)
    assert pert["loop"] == loop and _clears(pert["eps_history"], sc.FPM3)


# ---- the conditions on the reference alone, for every case of the device test ---------------------------------------------------
@pytest.mark.parametrize("row,key", pk.TRUNC_PARAMS, ids=pk.case_id)
def test_truncated_cases_can_be_compared(row, key):
    c = pk.trunc_case(row, key)
    for k in c.ks:
        want = [kr.truncated(r, k) for r in c.ref]
        assert 32.0 * c.drift[k] <= pk.POWER, (row, key, k, c.drift[k])
        assert sum(w[4] < pk.MARGIN_MIN for w in want) <= pk.LEFT_OUT_MAX * len(want)
        assert c.drift[k] > 0.0 or k <= 1                 # (the complex128 runs were compared at this k, not skipped)


@pytest.mark.parametrize("row,key,rtol", pk.STOP_PARAMS, ids=pk.case_id)
def test_stop_cases_can_be_compared(row, key, rtol):
    c = pk.stop_case(row, key, rtol)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= pk.LEFT_OUT_MAX * c.m
    assert 32.0 * c.drift.max() <= pk.POWER
    assert all(r.status == 0 and not r.active for r in c.ref)
    steps = {r.steps for r in c.ref}
    assert len(steps) >= (3 if rtol < 1e-2 else 2), steps            # the columns do stop at different steps


def test_gmres_case_can_be_compared():
    c = pk.gmres_case()
    for k in c.ks:
        assert 32.0 * c.drift[k] <= pk.POWER and c.drift[k] > 0.0
        assert all(w[4] >= pk.MARGIN_MIN and w[3] and w[1] == k for w in c.want[k])      # every column takes all k lock-steps
    assert c.products == {5: 7, 8: 10, 9: 12}           # cycle starts + steps + the closing start (restart 8)


@pytest.mark.parametrize("setting,shifted", pk.SWEEP_PARAMS, ids=pk.case_id)
def test_sweep_cases_can_be_compared(setting, shifted):
    c = pk.sweep_case(setting, shifted)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= pk.LEFT_OUT_MAX * c.decided.size
    assert 32.0 * c.drift <= pk.POWER, c.drift
    if setting[3] <= 50 and not shifted:
        assert (c.status == kr.NO_CONVERGENCE).any()      # the cap bites at a node


# ---- keyword validation: host only ------------------------------------------------------------------------------------------------
def _sparse(cplx=False):
    return list(sc.mixed_pattern_coeffs(sc.GRIDS[0], 2, cplx))


def _symmetric(kind):
    L = sc.laplacian(5, 4)
    I = sp.identity(20, format="csr")
    if kind == "complex-symmetric":
        return [L, sp.csr_matrix((0.1 + 0.3j) * L), I]
    if kind == "hermitian":
        H = sp.csr_matrix(L + 1j * (sp.triu(L, 1) - sp.tril(L, -1)))
        return [L, H, I]
    return [L, sp.csr_matrix(0.1 * I + 0.05 * L), I]


@pytest.mark.parametrize("coeffs,kw,word", [
    (_sparse(), {"solver": "bicgstab"}, 'method="projected"'),
    (_sparse(), {"solver": "gmres", "method": "linearised"}, 'method="projected"'),
    ([c.toarray() for c in _sparse()], {"solver": "bicgstab", "method": "projected"}, 'solver="direct"'),
    (_sparse()[:2] + [_sparse()[2].toarray()], {"solver": "cocg", "method": "projected"}, 'solver="direct"'),
    (_sparse(), {"solver": "cocg", "method": "projected"}, '"bicgstab"'),
    (_symmetric("hermitian"), {"solver": "cocg", "method": "projected"}, '"bicgstab"'),
    (_sparse(), {"solver": "bicgstab", "method": "projected", "solver_maxiter": 0}, "solver_maxiter"),
    (_sparse(), {"solver": "minres", "method": "projected"}, "solver"),
])
def test_krylov_keyword_validation_is_host_only(coeffs, kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    with pytest.raises(ValueError, match=word):
        fk.feast_polynomial(coeffs, 0.0, 1.0, M0=3, **kw)


def test_valid_krylov_keywords_reach_the_engine(monkeypatch):
    class Reached(Exception):
        pass

    def no_engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(fk.api, "_engine", no_engine)
    assert fk.api.POLY_KRYLOV_SOLVERS == ("bicgstab", "cocg", "gmres")
    for coeffs, kw in ((_sparse(), {"solver": "bicgstab"}), (_sparse(True), {"solver": "gmres", "solver_restart": 8}),
                       (_symmetric("real"), {"solver": "cocg", "solver_tol": 1e-4, "solver_maxiter": 50}),
                       (_symmetric("complex-symmetric"), {"solver": "cocg"})):
        with pytest.raises(Reached):
            fk.feast_polynomial(coeffs, 0.0, 1.0, M0=3, method="projected", **kw)
