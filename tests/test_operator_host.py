"""Operator handles without a GPU: the new entry point in the built library, every argument check of feast_matvec /
feast_general_matvec (all of them run before an engine is made or used), the host pieces of operator_cases.py, and -- for every
reference case that test_gpu_operator.py compares -- the project's own conditions on the reference alone: 32 D <= POWER and at
most LEFT_OUT_MAX of the (node, column) pairs undecided at MARGIN_MIN.  (The truncation cases are borrowed from
krylov_cases.py / gmres_cases.py; test_krylov_reference_host.py and test_gmres_reference_host.py assert the conditions for
their `dense` selections.)"""
import ctypes

import numpy as np
import pytest

import feastkit_jl_amd as fk
import krylov_cases as kc
import operator_cases as oc
from feastkit_jl_amd import _lib


class _NoEngine:
    """stands where the engine goes: a check that lets a bad argument through would touch it"""
    def __getattr__(self, name):
        raise AssertionError("the argument checks must run before the engine is used")


def _mul(Y, X):
    Y.copy_(X)


def test_symbol_is_declared_exported_and_refuses_a_null_handle():
    lib = fk.load_library()
    assert "feasthip_set_operator" in _lib.SYMBOLS
    assert isinstance(lib.feasthip_set_operator, ctypes._CFuncPtr)
    cb = _lib.APPLY_FN(lambda *a: 0)
    assert lib.feasthip_set_operator(None, 4, cb, None, 0) == 7
    assert (_lib.OP_B_IDENTITY, _lib.OP_COMPLEX, _lib.OP_SYMMETRIC) == (1, 2, 4)
    assert callable(fk.feast_matvec) and callable(fk.feast_general_matvec)


@pytest.mark.parametrize("kw,match", [
    (dict(solver="direct"), "Krylov solvers 'gmres', 'bicgstab'"),
    (dict(solver="lu"), "Krylov solvers 'gmres', 'bicgstab'"),
    (dict(solver="sparse_direct"), "Krylov solvers 'gmres', 'bicgstab'"),
    (dict(solver="banded"), "Krylov solvers 'gmres', 'bicgstab'"),
    (dict(solver="cocg"), "'bicgstab'"),
    (dict(solver="cocg", symmetric=False), "symmetric=True"),
    (dict(inner_precision=32), "inner_precision"),
    (dict(A_mul=np.eye(6)), "A_mul must be callable"),
    (dict(B_mul=np.eye(6)), "B_mul must be callable"),
    (dict(N=0), "N must be at least 1"),
    (dict(N=-3), "N must be at least 1"),
])
@pytest.mark.parametrize("general", [False, True], ids=["matvec", "general"])
def test_value_errors(general, kw, match):
    args = dict(A_mul=_mul, B_mul=None, N=6, M0=3, engine=_NoEngine())
    args.update(kw)
    A_mul, B_mul, N = args.pop("A_mul"), args.pop("B_mul"), args.pop("N")
    with pytest.raises(ValueError, match=match):
        if general:
            fk.feast_general_matvec(A_mul, B_mul, N, 0.5, 1.0, **args)
        else:
            fk.feast_matvec(A_mul, B_mul, N, (0.0, 1.0), **args)


def test_the_slicing_laplacian_has_the_closed_form_spectrum():
    L = oc.laplacian_matrix()
    assert L.shape == (960, 960) and abs(L - L.T).max() == 0
    lam = np.linalg.eigvalsh(L.toarray())
    assert np.abs(lam - oc.laplacian_eigenvalues()).max() <= 1e-12
    # the convection-diffusion operator is real and not symmetric
    C = oc.convection_diffusion()
    assert C.shape == (196, 196) and np.abs(C - C.T).max() > 0.1


def _conditions(c, real):
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= kc.LEFT_OUT_MAX * c.decided.size
    assert 32.0 * c.drift[real] <= kc.POWER, c.drift


@pytest.mark.parametrize("method,solver,rtol,maxit,warm", oc.SWEEPS)
def test_sweep_references_meet_the_conditions(method, solver, rtol, maxit, warm):
    c = oc.sweep_case(method, rtol, maxit, warm)
    _conditions(c, True)
    assert len(c.Z) == 8 and c.m == 24
    if maxit == 7:
        st = np.asarray(c.ref.status)
        assert (c.ref.steps == 7).any() and (st == 5).any()                             # the cap bites
    else:
        assert len(set(c.ref.steps.ravel())) >= 2                                       # mixed stops: columns leave at different steps


def test_gmres_sweep_reference_meets_the_conditions():
    c = oc.gmres_sweep_case()
    _conditions(c, True)
    assert len(c.ref.lock_steps) == 3           # batches of 3, 3 and 2 nodes
