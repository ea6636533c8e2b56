"""The per-column Krylov restatement (krylov_reference.py) checked against itself and against numpy.linalg.solve, and the
conditions on the inputs of test_gpu_krylov_steps.py (krylov_cases.py) that keep the device comparison from hiding a
failure: discriminating power (32 D <= 1e-7, D the drift of the restatement in complex128 against long double over four
summation orders) and decidable stops (at most 2 % of the (node, column) pairs of a case within 1e-6 of a stop
threshold).  No GPU."""
import numpy as np
import pytest

import feast_oracle as fo
import krylov_cases as kc
import krylov_reference as kr
from test_gpu_primitives import sparse_pair


def _solve_ref(A, B, z, b):
    A = A.toarray() if hasattr(A, "toarray") else A
    Bd = np.eye(A.shape[0]) if B is None else (B.toarray() if hasattr(B, "toarray") else B)
    return np.linalg.solve(z * Bd - A, b)


@pytest.mark.parametrize("method,cplx,bid", [("bicgstab", False, False), ("bicgstab", False, True), ("bicgstab", True, False),
                                             ("cocg5", False, False), ("cocg5", False, True),
                                             ("cocg_fused", False, False), ("cocg_fused", False, True)])
def test_converged_restatement_meets_direct_solve(method, cplx, bid):
    N = 60
    A, B = sparse_pair(N, 3, cplx=cplx, b_identity=bid)
    z = -3.0 + 2.0j
    rng = np.random.default_rng(4)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    for dtype, tol in ((np.clongdouble, 1e-11), (np.complex128, 1e-10)):
        col = kr.solve_column(kr.Pencil(A, B, dtype), z, b, method, 1e-13, 0.0, 500)
        assert col.status == 0 and not col.active and 0 < col.steps < 500
        assert col.rnorm <= 1e-13 * col.r0norm
        assert kr.rel_dist(col.x.astype(np.complex128), _solve_ref(A, B, z, b)) <= tol


def test_fused_and_five_launch_cocg_agree_in_long_double():
    """rho' = alpha^2 kappa - rho is r'^T r' when r^T q = p^T q: in long double both forms give the same iterates for
    k <= 48 on the 12 x 10 x 9 cfg-3 pencil, every node of the 8-node contour (the claim the fused form rests on)."""
    A, B, Z, W, _ = kc.sweep_problem()
    P = kr.Pencil(A, B, np.clongdouble)
    b = P.mulB(kc.fk.seeded_subspace(A.shape[0], 4)[:, 1].astype(np.clongdouble))
    near = int(np.argmin(np.abs(Z.imag)))
    for e, z in enumerate(Z):
        f = kr.solve_column(P, z, b, "cocg_fused", 1e-14, 0.0, 48, keep_history=True)
        g = kr.solve_column(P, z, b, "cocg5", 1e-14, 0.0, 48, keep_history=True)
        assert f.steps == g.steps == 48 and f.active and g.active
        worst = max(kr.rel_dist(f.history[k][0], g.history[k][0]) for k in range(1, 49))
        assert worst <= (1e-13 if e == near else 1e-17), (e, worst)


def test_edge_rules():
    A, B = sparse_pair(40, 6)
    P = kr.Pencil(A, B, np.clongdouble)
    z = -3.0 + 2.0j
    b = np.random.default_rng(1).standard_normal(40)
    for method in kr.METHODS:
        zero = kr.solve_column(P, z, np.zeros(40), method, 1e-3, 0.0, 50)
        assert zero.steps == 0 and zero.status == 0 and not zero.active and not zero.x.any()
        x0 = np.arange(40.0)
        masked = kr.solve_column(P, z, b, method, 1e-3, 0.0, 50, x0=x0, masked=True)
        assert masked.steps == 0 and not masked.active and np.array_equal(masked.x, x0)
        one = kr.solve_column(P, z, b, method, 1e-14, 0.0, 1, keep_history=True)
        assert one.steps == 1 and one.active and one.status == 0
        assert kr.node_status([one], 1e-14, 0.0) == kr.NO_CONVERGENCE
        more = kr.solve_column(P, z, b, method, 1e-14, 0.0, 9, keep_history=True)
        assert kr.rel_dist(more.history[1][0], one.x) == 0.0          # maxit only cuts the same sequence short
        x, steps, status, active, _ = kr.truncated(more, 1)
        assert steps == 1 and active and np.array_equal(x, one.x)
        bad = b.copy(); bad[3] = np.nan
        nan = kr.solve_column(P, z, bad, method, 1e-3, 0.0, 50)
        assert nan.status == kr.BREAKDOWN and nan.steps == 0 and not nan.active
        assert kr.node_status([nan], 1e-3, 0.0) == kr.NO_CONVERGENCE     # never "converged"
        tiny = kr.solve_column(P, z, 1e-9 * b / np.linalg.norm(b), method, 3e-2, 1e-6, 50)
        assert tiny.steps == 0 and tiny.status == 0 and not tiny.active
    # p^T S p = 0 (exactly) on a complex-symmetric 2 x 2 example: S = -A = diag(-1 - i, 1 + i), p = r0 = (1, 1), rho = 2
    A2 = np.diag([1.0 + 1.0j, -1.0 - 1.0j])
    for method in ("cocg5", "cocg_fused"):
        brk = kr.solve_column(kr.Pencil(A2, None, np.clongdouble), 0.0, np.array([1.0, 1.0]), method, 1e-3, 0.0, 50)
        assert brk.status == kr.BREAKDOWN and not brk.active and brk.steps == 0
        assert kr.node_status([brk], 1e-3, 0.0) == kr.NO_CONVERGENCE


def test_predicted_stop_rule():
    """rtol >= 1e-3 and atol == 0: a fused column stops on the estimate, takes that step, and reports the estimate; with
    atol > 0 or rtol < 1e-3 it stops on the true norm one product late and never before the five-launch form."""
    A, B, Z, W, _ = kc.sweep_problem()
    P = kr.Pencil(A, B, np.clongdouble)
    b = P.mulB(kc.fk.seeded_subspace(A.shape[0], 4)[:, 0].astype(np.clongdouble))
    z = Z[5]
    pred = kr.solve_column(P, z, b, "cocg_fused", 3e-2, 0.0, 200)
    five = kr.solve_column(P, z, b, "cocg5", 3e-2, 0.0, 200)
    assert pred.status == five.status == 0 and pred.steps == five.steps
    assert kr.rel_dist(pred.x, five.x) <= 1e-15
    assert abs(pred.rnorm / five.rnorm - 1.0) <= 1e-10            # cfg 3 with a real right-hand side: the estimate is exact
    off = kr.solve_column(P, z, b, "cocg_fused", 3e-2, 1e-300, 200)
    assert off.steps == five.steps and kr.rel_dist(off.x, five.x) <= 1e-15


@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("name", kc.TRUNC_HOST)
def test_truncated_inputs_have_discriminating_power(name, near):
    c = kc.trunc_case(name, near)
    for k in c.ks:
        assert 32.0 * c.drift[k] <= kc.POWER, (name, near, k, c.drift[k])


def test_stop_inputs_stop_at_different_steps_and_are_decidable():
    for solver, method, dense in kc.STOP_SOLVERS:
        for rtol, atol in kc.STOP_SETTINGS:
            c = kc.stop_case(method, rtol, atol)
            steps = [r.steps for r in c.ref]
            assert steps[5] == 0 and not c.ref[5].x.any()                     # the zero column
            if atol > 0:
                assert steps[11] == 0 and c.ref[11].r0norm <= atol            # below atol from the start
            assert len(set(steps)) >= 6, steps                                 # clearly different steps
            assert all(r.status == 0 and not r.active for r in c.ref)
            assert c.decided.all(), (method, rtol, atol, [r.margin for r in c.ref])
            assert c.fp64_steps_agree
            assert 32.0 * c.drift.max() <= kc.POWER, (method, rtol, atol, c.drift.max())


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("rtol,maxit", kc.SWEEP_SETTINGS)
def test_sweep_inputs_are_decidable_and_discriminating(rtol, maxit, warm):
    c = kc.sweep_case("cocg_fused", rtol, maxit, 24, warm)
    assert c.decided.all()                       # the reference alone leaves out no pair
    assert c.fp64_steps_agree
    for real in (True, False):
        assert 32.0 * c.drift[real] <= kc.POWER, (rtol, maxit, warm, real, c.drift[real])
    if (rtol, maxit) == (1e-3, 60):
        # the node nearest Emax is capped at 60 steps, the others converge
        assert list(c.ref.status) == [0] * 7 + [kr.NO_CONVERGENCE] and c.ref.steps[7].max() == 60


@pytest.mark.parametrize("kind,real,maxit", kc.BICGSTAB_SWEEPS[1:])
def test_bicgstab_sweep_inputs_are_decidable_and_discriminating(kind, real, maxit):
    c = kc.sweep_case("bicgstab", 3e-2, maxit, 24, True, kind=kind)
    assert c.decided.all() and c.fp64_steps_agree
    assert 32.0 * max(c.drift.values()) <= kc.POWER, c.drift
    assert len(set(c.ref.steps.ravel())) >= 2
