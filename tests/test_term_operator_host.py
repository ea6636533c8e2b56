"""Term operators without a GPU: every argument check of feast_nonlinear_matvec / feast_polynomial_matvec (all of them run
before an engine is made or used), the new entry points in the built library, the restatement TermOp against the dense T(z) in
long double, and -- for every reference case test_gpu_term_operator.py compares the device with -- the project's conditions on
the reference alone: the four fp64 summation orders take the long-double run's steps, 32 D stays inside the discriminating
power, and at most 2 % of the (node, column) pairs are decided by less than the margin."""
import ctypes

import numpy as np
import pytest

import feastkit_jl_amd as fk
import krylov_reference as kr
import nonlinear_cases as nc
import nonlinear_reference as nr
import term_operator_cases as tc
from feastkit_jl_amd import _lib

NEW_SYMBOLS = ("feasthip_set_term_operator", "feasthip_set_term_norms")


class _NoEngine:
    """stands where the engine goes: a check that lets a bad argument through would touch it"""
    def __getattr__(self, name):
        raise AssertionError("the argument checks must run before the engine is used")


def _mul(Y, X):
    Y.copy_(X)


def _terms(n=3):
    return [(_mul, 0), (None, lambda z: -z), (_mul, nc.exp_term(1.0)), (_mul, 2), (_mul, 3)][:n]


def test_symbols_are_declared_and_exported():
    lib = fk.load_library()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert callable(fk.feast_nonlinear_matvec) and callable(fk.feast_polynomial_matvec)
    assert hasattr(fk.HipEngine, "set_term_operator") and hasattr(fk.HipEngine, "set_term_norms")


def test_null_handles_are_refused():
    lib = fk.load_library()
    cb = _lib.APPLY_FN(lambda *a: 0)
    assert lib.feasthip_set_term_operator(None, 4, 2, cb, None, 0, 0, 0) == 7
    assert lib.feasthip_set_term_norms(None, None) == 7


KRYLOV_NAMES = "'gmres', 'bicgstab' or .* 'cocg'"


@pytest.mark.parametrize("make,match", [
    (lambda: dict(solver="direct"), KRYLOV_NAMES),
    (lambda: dict(solver="sparse_direct"), KRYLOV_NAMES),
    (lambda: dict(solver="banded"), KRYLOV_NAMES),
    (lambda: dict(solver="shifted_cocg"), KRYLOV_NAMES),
    (lambda: dict(solver="cocg"), "symmetric=True"),
    (lambda: dict(M0="auto"), "count estimate"),
    (lambda: dict(terms=_terms(1)), "2 to 9 terms"),
    (lambda: dict(terms=_terms(5) * 2), "2 to 9 terms"),
    (lambda: dict(terms=[(np.eye(12), 0), (_mul, 1)]), "callable"),
    (lambda: dict(terms=[(_mul,), (_mul, 1)]), "pair"),
    (lambda: dict(N=0), "N must be at least 1"),
    (lambda: dict(terms=[(_mul, 0), (_mul, lambda z: 1.0 / (z - z))]), "not finite at a contour node"),
    (lambda: dict(terms=[(_mul, 0), (_mul, "exp")]), "callable or a non-negative int"),
    (lambda: dict(norms=[1.0, 2.0]), "norms"),
    (lambda: dict(norms=[1.0, 0.0, 2.0]), "norms"),
    (lambda: dict(norms=[1.0, -1.0, 2.0]), "norms"),
    (lambda: dict(radius=0.0), "radius"),
    (lambda: dict(Q0=np.ones((12, 3))), "Q0"),
    (lambda: dict(moments=0), "moments"),
    (lambda: dict(ortho="householder"), "ortho"),
])
def test_value_errors_of_feast_nonlinear_matvec(make, match):
    kw = dict(terms=_terms(), N=12, center=0.5, radius=1.0, M0=4, engine=_NoEngine())
    kw.update(make())
    terms, N, center, radius = kw.pop("terms"), kw.pop("N"), kw.pop("center"), kw.pop("radius")
    with pytest.raises(ValueError, match=match):
        fk.feast_nonlinear_matvec(terms, N, center, radius, **kw)


@pytest.mark.parametrize("make,match", [
    (lambda: dict(solver="direct"), KRYLOV_NAMES),
    (lambda: dict(solver="lu"), KRYLOV_NAMES),
    (lambda: dict(solver="cocg"), "symmetric=True"),
    (lambda: dict(M0="auto"), "count estimate"),
    (lambda: dict(muls=[_mul]), "2 to 9 terms"),
    (lambda: dict(muls=[_mul] * 10), "2 to 9 terms"),
    (lambda: dict(muls=[_mul, 3.0]), "callable"),
    (lambda: dict(N=-2), "N must be at least 1"),
    (lambda: dict(norms=[1.0]), "norms"),
    (lambda: dict(norms=[1.0, np.inf, 1.0]), "norms"),
])
def test_value_errors_of_feast_polynomial_matvec(make, match):
    kw = dict(muls=[_mul, None, _mul], N=12, center=0.5, radius=1.0, M0=4, engine=_NoEngine())
    kw.update(make())
    muls, N, center, radius = kw.pop("muls"), kw.pop("N"), kw.pop("center"), kw.pop("radius")
    with pytest.raises(ValueError, match=match):
        fk.feast_polynomial_matvec(muls, N, center, radius, **kw)
    assert "moments" not in fk.feast_polynomial_matvec.__kwdefaults__ and "reduced_nodes" not in fk.feast_polynomial_matvec.__kwdefaults__


def test_the_existing_refusals_stand():
    """feast_nonlinear keeps its "out of scope" for Krylov solvers on matrices, feast_matvec its checks"""
    I = np.eye(6)
    with pytest.raises(ValueError, match="out of scope"):
        fk.feast_nonlinear([(I, 0), (I, 1)], 0.0, 1.0, solver="gmres", engine=_NoEngine())
    with pytest.raises(ValueError, match="needs a matrix to factor"):
        fk.feast_matvec(_mul, None, 6, (0.0, 1.0), solver="direct", engine=_NoEngine())


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("nt", [2, 3, 9])
def test_termop_apply_is_the_dense_product(nt, cplx):
    """TermOp.apply in long double against T(z) x with T formed densely in long double: within 8 nt N eps_ld sum_k |f_k| ||A_k||_F ||x||
    (the rounding of nt products of N terms each in long double); in complex128 within the same with eps of float64."""
    N = 63
    mats, X, _ = tc.product_inputs(N, 7, nt, cplx)
    funcs = [f for _, f in nc.random_terms(4, 9, False)][:nt]
    z = 0.3 - 0.7j
    T = tc.dense_t(mats, funcs, z)
    scale = float(np.abs(nr.table(funcs, [z])[0]) @ np.array(tc.exact_norms(mats)))
    for dtype in (np.clongdouble, np.complex128):
        op = tc.TermOp(mats, funcs, dtype)
        assert op.N == N and op.dtype == np.dtype(dtype) and op.real == np.zeros(1, dtype).real.dtype
        eps = float(np.finfo(op.real).eps)
        for j in range(3):
            err = float(np.linalg.norm((op.apply(z, X[:, j]).astype(np.clongdouble) - T @ X[:, j].astype(np.clongdouble))))
            assert err <= 8 * nt * N * eps * scale * np.linalg.norm(X[:, j]), (nt, cplx, dtype, err)


def test_termop_leaves_out_a_term_with_a_zero_scalar():
    mats, X, _ = tc.product_inputs(63, 7, 3, False)
    op = tc.TermOp([mats[0], None, np.full((63, 63), np.nan)], [lambda z: np.ones_like(z), lambda z: -z, lambda z: 0.0 * z], np.complex128)
    y = op.apply(2.0 + 1.0j, X[:, 0])
    assert np.isfinite(y).all() and np.allclose(y, mats[0] @ X[:, 0] - (2.0 + 1.0j) * X[:, 0])


# ---- the conditions on the references alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("solver", ["bicgstab", "cocg"])
def test_truncation_references(solver, near):
    c = tc.trunc_case(solver, near)
    for k in c.ks:
        want = [kr.truncated(r, k) for r in c.ref]
        assert sum(w[4] < tc.MARGIN_MIN for w in want) <= tc.LEFT_OUT_MAX * len(want)
        assert 32.0 * c.drift[k] <= tc.POWER, (solver, near, k, c.drift[k])


@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
def test_gmres_truncation_references(near):
    c = tc.gmres_case(near)
    for k in c.ks:
        assert all(w[4] >= tc.MARGIN_MIN for w in c.want[k])
        assert 32.0 * c.drift[k] <= tc.POWER, (near, k, c.drift[k])


@pytest.mark.parametrize("setting,shifted", tc.SWEEP_PARAMS, ids=lambda p: "-".join(str(x) for x in p) if isinstance(p, tuple) else str(p))
def test_sweep_references(setting, shifted):
    c = tc.sweep_case(setting, shifted)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= tc.LEFT_OUT_MAX * c.decided.size
    assert 32.0 * c.drift[False] <= tc.POWER, (setting, shifted, c.drift)
    if setting[2] == 1e-4 and not shifted:          # the nodes leave at different steps, none is capped
        rowmax = c.steps.max(axis=1)
        assert not c.status.any() and rowmax.min() < rowmax.max() < 400


@pytest.mark.parametrize("name", tc.DRIVER_NAMES)
def test_inexact_driver_converges(name):
    mats, funcs, case, _, _ = tc.driver_case(name)
    ref, again = tc.driver_run(name), tc.driver_run(name, 1e-14)
    err = nr.match_error(ref["lam"], case["lam_in"]) if ref["M"] == case["count"] else np.inf
    print("inexact driver %s: loop %d (perturbed %d) history %s eigenvalue error %.2e" % (name, ref["loop"], again["loop"],
                                                                                      ["%.1e" % e for e in ref["eps_history"]], err))
    assert ref["info"] == 0 and ref["M"] == case["count"] and again["info"] == 0 and again["loop"] == ref["loop"]
    assert err <= 1e-8
