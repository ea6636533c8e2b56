"""Krylov solves on P(z) for sparse coefficients on the device (feast_polynomial(..., solver="bicgstab" | "cocg" | "gmres"),
csrc/fh_poly.hip: k_spmm_poly under the batched drivers of csrc/fh_api.hip): the operator product against the dense one,
truncated solves and own stop steps against the step-exact long-double references (krylov_reference / gmres_reference on
polynomial_krylov_reference.PolyOp), inexact sweeps against the per-column restatement, the driver against the inexact
restatement of the projected method, and the refusals at the C ABI.

The comparisons with the references are those of test_gpu_krylov_steps.py: D = the drift of the restatement itself in
complex128 over four summation orders against long double, the device must lie within max(32 D, 64 eps)
(krylov_reference.tolerance) and 32 D <= 1e-7 is asserted for every compared case; (node, column) pairs whose stop is decided
by less than 1e-6 are left out, at most 2 % of a case.  test_polynomial_krylov_host.py asserts those conditions on the
reference alone."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feast_oracle as fo
import feastkit_jl_amd as fk
import krylov_reference as kr
import polynomial_krylov_reference as pk
import polynomial_projected_reference as ppr
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd.ingest import polynomial_union_csr
from feastkit_jl_amd.types import FeastHipError

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FPM_ERROR = 9


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")
    engine.set_ortho_method("mgs")


def _setup(engine, coeffs, contour=None):
    engine.set_adjoint(False)
    engine.set_polynomial_csr(*polynomial_union_csr(coeffs))
    engine.set_real_projection(False)
    if contour is not None:
        engine.set_contour(contour[0], contour[1], 1.0)


def _fpm(fpm3, ne):
    fpm = fk.feastinit()
    fpm[8], fpm[3] = ne, fpm3
    return fpm


def close_enough(group, dist, D):
    print("poly-krylov %s D=%.3e device=%.3e tol=%.3e" % (group, D, dist, kr.tolerance(D)))
    assert 32.0 * D <= pk.POWER, (group, D)              # a condition on the reference alone
    assert dist <= kr.tolerance(D), (group, dist, D)


# ---- the operator product ------------------------------------------------------------------------------------------------------
PRODUCT_Z = np.array([pk.FAR_Z, 3.0 - 2.0j, -4.0 + 1.0j])         # |z| up to 4.1: a_k z^k of the highest degree stays far above rounding


def _product_check(engine, coeffs, d, m, tag):
    """Y_e = P(z_e) X_e, B - P(z_e) X_e (B shared) and B_e - P(z_e) X_e for 3 nodes, each within 16 d N eps ||P(z_e)||_F ||X_e||_F
    of the product formed in long double (the bound DESIGN.md section 6p uses for its products)."""
    N = coeffs[0].shape[0]
    ne = len(PRODUCT_Z)
    _setup(engine, coeffs, (PRODUCT_Z, np.ones(ne, dtype=complex)))
    engine.set_solver("direct")
    X = [sc.random_block(N, m, 50 + e) for e in range(ne)]
    B = [sc.random_block(N, m, 60 + e) * 5.0 for e in range(ne)]
    dX = engine.upload(np.concatenate(X, axis=1))
    P = [sum((sp.csr_matrix(c).astype(np.complex128) * z ** k for k, c in enumerate(coeffs)), sp.csr_matrix((N, N), dtype=np.complex128))
         for z in PRODUCT_Z]
    if N <= 400:          # the dense product in long double; beyond: scipy's in complex128, whose own error is far inside the bound
        want = [pk.dense_poly(coeffs, PRODUCT_Z[e]) @ X[e].astype(np.clongdouble) for e in range(ne)]
    else:
        want = [np.asarray(P[e] @ X[e]) for e in range(ne)]
    bound = [16 * d * N * EPS * spla.norm(P[e]) * np.linalg.norm(X[e]) for e in range(ne)]
    for name, dB, ref in (("PX", None, want),
                          ("B-PX", engine.upload(B[0]), [B[0] - w for w in want]),
                          ("Be-PX", engine.upload(np.concatenate(B, axis=1)), [B[e] - want[e] for e in range(ne)])):
        Y = engine.download(engine.poly_node_products(dX, m, dB))
        for e in range(ne):
            err = float(np.linalg.norm((Y[:, e * m:(e + 1) * m] - ref[e]).astype(np.clongdouble)))
            print("poly-krylov product/%s/%s/node=%d err=%.3e bound=%.3e" % (tag, name, e, err, bound[e]))
            assert err <= bound[e], (tag, name, e, err, bound[e])


@pytest.mark.parametrize("m", [7, 24, 40])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_operator_product(engine, restore, d, cplx, m):
    """N = 63, a multiple of no tile; panel widths 16, 32 and 64; real and complex values"""
    _product_check(engine, sc.mixed_pattern_coeffs(sc.GRIDS[0], d, cplx), d, m, "N=63/d=%d/%s/m=%d" % (d, "c" if cplx else "r", m))


def test_operator_product_beyond_one_grid_pass(engine, restore):
    """N = 4200 under 64-lane row slices: the 1024 workgroups take 4096 rows per pass"""
    _product_check(engine, pk._operator(pk.BIG)[0], 2, 40, "N=4200/d=2/r/m=40")


def test_node_products_need_a_sparse_handle_and_a_narrow_block(engine, restore):
    dense = sc.dense(sc.mixed_pattern_coeffs(sc.GRIDS[0], 2, False))
    engine.set_polynomial(dense)
    engine.set_solver("direct")
    engine.set_contour(PRODUCT_Z, np.ones(3, dtype=complex), 1.0)
    with pytest.raises(FeastHipError) as err:
        engine.poly_node_products(engine.upload(sc.random_block(63, 6, 1)), 2)
    assert err.value.code == FPM_ERROR and "CSR" in str(err.value)
    _setup(engine, sc.mixed_pattern_coeffs(sc.GRIDS[1], 2, False), (PRODUCT_Z[:1], np.ones(1, dtype=complex)))
    with pytest.raises(FeastHipError) as err:
        engine.poly_node_products(engine.upload(sc.random_block(286, 65, 1)), 65)
    assert err.value.code == 2


# ---- truncated solves and own stop steps, through feasthip_poly_solve_dev -----------------------------------------------------------
@pytest.mark.parametrize("row,key", pk.TRUNC_PARAMS, ids=pk.case_id)
def test_truncated_solve_is_the_kth_iterate(engine, restore, row, key):
    """maxit = k, rtol = 1e-14: rc 5 and Y is the reference's k-th iterate, krylov_iterations = k; where the reference reaches
    the target before step k: rc 0, its stop step and its iterate at that step."""
    c = pk.trunc_case(row, key)
    _setup(engine, c.coeffs)
    dX = engine.upload(c.X)
    for k in c.ks:
        engine.set_solver(c.solver, rtol=1e-14, atol=0.0, maxit=k)
        dY, rc = engine.poly_solve(c.z, dX, c.m)
        Y = engine.download(dY)
        st = engine.last_stats
        want = [kr.truncated(r, k) for r in c.ref]       # (x, steps, status, active, margin)
        decided = [w[4] >= pk.MARGIN_MIN for w in want]
        assert sum(not d for d in decided) <= pk.LEFT_OUT_MAX * len(want)
        if all(decided):
            assert rc == (kr.NO_CONVERGENCE if any(w[3] for w in want) else 0), (row, key, k, rc)
            assert st["krylov_iterations"] == max(w[1] for w in want), (row, key, k, st)
            assert list(engine.last_column_iterations(1, c.m)[0]) == [w[1] for w in want]
            assert st["factorizations"] == 0
        dist = max(kr.rel_dist(Y[:, j], w[0]) for j, (w, ok) in enumerate(zip(want, decided)) if ok)
        close_enough("truncated/%s/k=%d" % (pk.case_id((row, key)), k), dist, c.drift[k])


@pytest.mark.parametrize("row,key,rtol", pk.STOP_PARAMS, ids=pk.case_id)
def test_every_column_stops_at_its_own_step(engine, restore, row, key, rtol):
    """Each column of Y is the reference iterate at that column's own stop step"""
    c = pk.stop_case(row, key, rtol)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= pk.LEFT_OUT_MAX * c.m
    _setup(engine, c.coeffs)
    engine.set_solver(c.solver, rtol=rtol, atol=0.0, maxit=pk.STOP_MAXIT)
    dY, rc = engine.poly_solve(c.z, engine.upload(c.X), c.m)
    Y = engine.download(dY)
    assert rc == 0
    counts = engine.last_column_iterations(1, c.m)[0]
    assert np.array_equal(counts[c.decided], np.array([r.steps for r in c.ref])[c.decided]), (counts, [r.steps for r in c.ref])
    if c.decided.all():
        assert engine.last_stats["krylov_iterations"] == max(r.steps for r in c.ref)
        assert list(engine.last_node_iterations(1)) == [max(r.steps for r in c.ref)]
    for j in np.flatnonzero(c.decided):
        close_enough("stops/%s/col=%d/step=%d" % (pk.case_id((row, key, rtol)), j, c.ref[j].steps), kr.rel_dist(Y[:, j], c.ref[j].x), c.drift[j])


def test_gmres_truncated_iterate_and_product_count(engine, restore):
    """GMRES(8) on the N = 286 mixed quadratic, cut inside a cycle, on its boundary and one step after it"""
    c = pk.gmres_case()
    _setup(engine, c.coeffs)
    dX = engine.upload(c.X)
    for k in c.ks:
        engine.set_solver("gmres", rtol=1e-14, atol=0.0, maxit=k, restart=c.restart)
        dY, rc = engine.poly_solve(c.z, dX, c.m)
        Y = engine.download(dY)
        st = engine.last_stats
        want = c.want[k]
        assert all(w[4] >= pk.MARGIN_MIN for w in want)
        assert rc == kr.NO_CONVERGENCE and st["krylov_iterations"] == k and st["spmm_calls"] == c.products[k], (k, rc, st, c.products[k])
        assert list(engine.last_column_iterations(1, c.m)[0]) == [w[1] for w in want]
        close_enough("gmres/k=%d" % k, max(kr.rel_dist(Y[:, j], w[0]) for j, w in enumerate(want)), c.drift[k])


# ---- inexact sweeps, through feasthip_poly_resinv_apply_dev -------------------------------------------------------------------------
@pytest.mark.parametrize("setting,shifted", pk.SWEEP_PARAMS, ids=pk.case_id)
def test_inexact_sweep(engine, restore, setting, shifted):
    """The summed block of the plain (sigma None) and the residual-inverse sweep, the per-node status (5 where the cap bites),
    the per-column step counts over the decided pairs, the node counts and the statistics"""
    c = pk.sweep_case(setting, shifted)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= pk.LEFT_OUT_MAX * c.decided.size
    ne, m = len(c.Z), pk.SWEEP_M
    _setup(engine, c.coeffs, (c.Z, c.W))
    engine.set_solver(c.solver, rtol=c.rtol, atol=0.0, maxit=c.maxit)
    dQ, status, st = engine.poly_resinv_apply(engine.upload(c.X), m, c.sigma)
    out = engine.download(dQ, m)
    ok = np.flatnonzero(c.col_ok)
    close_enough("sweep/%s" % pk.case_id((setting, shifted)), kr.block_dist(out[:, ok], c.out[:, ok]), c.drift)
    counts = engine.last_column_iterations(ne, m)
    assert np.array_equal(counts[c.decided], c.steps[c.decided]), (counts, c.steps)
    assert st["factorizations"] == 0
    if c.decided.all():
        rowmax = c.steps.max(axis=1)
        assert list(status[:ne]) == list(c.status), (status, c.status)
        assert list(engine.last_node_iterations(ne)) == list(rowmax)
        assert st["krylov_iterations"] == rowmax.sum()


def _converged_sweep_check(tag, coeffs, Z, W, X, out, rtol):
    """A plain sweep whose solves all passed the stop test ||r|| <= rtol ||b||: node e's column j is within ||P(z_e)^-1||_2 rtol ||x_j||
    of the exact solve, so the summed block lies within sum_e |w_e| ||P(z_e)^-1||_2 rtol ||X||_F of the exact-solve sweep (twice
    that is allowed: BiCGStab tests its recurrence residual, which rounding parts from the true one far below rtol)."""
    dense = sc.dense(coeffs)
    inv = [np.linalg.norm(np.linalg.inv(pr.poly_at(dense, z)), 2) for z in Z]
    bound = 2.0 * rtol * np.linalg.norm(X) * sum(abs(w) * n for w, n in zip(W, inv))
    err = float(np.linalg.norm(out - ppr.sweep(dense, Z, W, X)))
    print("poly-krylov %s err=%.3e bound=%.3e" % (tag, err, bound))
    assert err <= bound, (tag, err, bound)


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _run(engine, name, scaled, solver, **kw):
    columns, seed, _ = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    Q0 = fo.seeded_subspace(case["N"], columns, seed)
    return fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=columns, fpm=_fpm(sc.FPM3, sc.NE), engine=engine, Q0=Q0,
                               solver=solver, method="projected", **kw)


@pytest.mark.parametrize("name,scaled,method,solver,rtol", pk.INEXACT_PINS, ids=pk.INEXACT_IDS)
def test_driver_on_inexact_solves(engine, restore, name, scaled, method, solver, rtol):
    columns, seed, loop = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    ref = pk.inexact_run(name, scaled, method, rtol)
    exact = ppr.damped_run(name, scaled, columns, seed)
    res = _run(engine, name, scaled, solver, solver_tol=rtol, solver_maxiter=2000)
    poly = res.stats["polynomial"]
    err = pr.match_error(res.lambda_, case["lam_in"]) if res.M == case["k"] else np.inf
    print("poly-krylov driver %s: loop %d history %s restatement %s exact %s worst column steps %s (restatement %s) eigenvalue error %.2e" % (
        solver, res.loop, ["%.2e" % e for e in poly["eps_history"]], ["%.2e" % e for e in ref["eps_history"]],
        ["%.2e" % e for e in exact["eps_history"]], [k["iterations"] for k in poly["krylov"]], [k["iterations"] for k in ref["krylov"]], err))
    assert res.info == 0 and res.M == ref["M"] == case["k"] and res.loop == ref["loop"] == loop
    assert err <= 1e-8
    for a, b in zip(poly["eps_history"], exact["eps_history"]):
        assert b / pk.HISTORY_FACTOR <= a <= b * pk.HISTORY_FACTOR, (poly["eps_history"], exact["eps_history"])
    assert res.stats["factorizations"] == 0
    assert poly["plan"] == "krylov" and poly["fell_back"] is False and "solver_substitution" not in res.stats
    assert not any(key.startswith("plan_") for key in poly)
    assert len(poly["krylov"]) == res.loop + 1
    for entry in poly["krylov"]:
        assert entry["capped_nodes"] == 0 and len(entry["node_iterations"]) == sc.NE and entry["iterations"] == max(entry["node_iterations"])
    assert res.stats["krylov_iterations"] == sum(sum(e["node_iterations"]) for e in poly["krylov"])


def test_driver_goes_on_when_the_cap_bites(engine, restore):
    """solver_maxiter = 20: every node stops at the cap in the early loops, which is counted and is no error"""
    res = _run(engine, "20x16", False, "bicgstab", solver_tol=1e-4, solver_maxiter=20)
    kry = res.stats["polynomial"]["krylov"]
    print("poly-krylov capped: info %d loop %d M %d history %s capped %s" % (res.info, res.loop, res.M, ["%.1e" % e for e in res.stats["polynomial"]["eps_history"]],
                                                                           [k["capped_nodes"] for k in kry]))
    assert res.info in (0, int(fk.FeastError.Feast_ERROR_NO_CONVERGENCE)) and res.M > 0
    assert len(kry) == res.loop + 1 and kry[0]["capped_nodes"] == sc.NE and all(k["iterations"] <= 20 for k in kry)
    assert res.stats["factorizations"] == 0


def test_cocg_and_bicgstab_agree(engine, restore):
    a = _run(engine, "20x16", False, "cocg", solver_tol=1e-4, solver_maxiter=2000)
    b = _run(engine, "20x16", False, "bicgstab", solver_tol=1e-4, solver_maxiter=2000)
    assert a.info == 0 and b.info == 0 and a.M == b.M
    assert pr.match_error(a.lambda_, b.lambda_) <= 1e-9


def test_gmres_sweep_solves(engine, restore):
    """GMRES over a batch of nodes: the plain sweep on the N = 286 mixed cubic at rtol = 1e-10 is the exact-solve sweep"""
    coeffs = sc.mixed_pattern_coeffs(sc.GRIDS[1], 3, True)
    Z, W = fo.feast_gcontour(*sc.sweep_circle(sc.GRIDS[1]), 8)
    X = sc.random_block(coeffs[0].shape[0], 7, 33)
    _setup(engine, coeffs, (Z, W))
    engine.set_solver("gmres", rtol=1e-10, atol=0.0, maxit=400, restart=30)
    dQ, status, st = engine.poly_resinv_apply(engine.upload(X), 7)
    assert not status.any() and st["krylov_iterations"] > 0 and st["factorizations"] == 0
    _converged_sweep_check("gmres-sweep", coeffs, Z, W, X, engine.download(dQ, 7), 1e-10)


# ---- errors at the C ABI ----------------------------------------------------------------------------------------------------------
def test_abi_refusals(engine, restore):
    coeffs = sc.mixed_pattern_coeffs(sc.GRIDS[0], 2, False)
    N, m = coeffs[0].shape[0], 5
    Z, W = fo.feast_gcontour(*sc.sweep_circle(sc.GRIDS[0]), 8)
    X = sc.random_block(N, m, 29)
    # a Krylov kind on a dense polynomial handle
    engine.set_polynomial(sc.dense(coeffs))
    engine.set_solver("direct")
    engine.set_contour(Z, W, 1.0)
    for solver in ("bicgstab", "cocg", "gmres"):
        with pytest.raises(FeastHipError) as err:
            engine.set_solver(solver)
        assert err.value.code == FPM_ERROR and "FEASTHIP_SOLVER_LU" in str(err.value)
    dY, rc = engine.poly_solve(0.5j, engine.upload(X), m)           # the handle stays usable, under the LU it had
    assert rc == 0 and kr.rel_dist(engine.download(dY), np.linalg.solve(pk.dense_poly(coeffs, 0.5j, np.complex128), X)) <= 1e-10
    # a Krylov kind set on a pencil, then a dense polynomial installed: the poly_ call itself refuses
    engine.set_problem(np.diag(np.arange(1.0, 9.0)))
    engine.set_solver("bicgstab")
    engine.set_polynomial(sc.dense(coeffs))
    with pytest.raises(FeastHipError) as err:
        engine.poly_solve(0.5j, engine.upload(X), m)
    assert err.value.code == FPM_ERROR and "FEASTHIP_SOLVER_LU" in str(err.value)
    # sparse handle: what stays refused, and the linearised sweep under a Krylov solver
    _setup(engine, coeffs, (Z, W))
    for call in (lambda: engine.set_solver("shifted_cocg"), lambda: engine.set_solver("block_cocg"), lambda: engine.set_solver("banded"),
                 lambda: engine.set_solver("bicgstab", factor_precision=32)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "polynomial" in str(err.value)
    engine.set_solver("bicgstab", rtol=1e-10, atol=0.0, maxit=400)
    with pytest.raises(FeastHipError) as err:
        engine.poly_contour_apply(engine.upload(sc.random_block(2 * N, m, 31)), m)
    assert err.value.code == FPM_ERROR and "projected" in str(err.value)
    dQ, status, st = engine.poly_resinv_apply(engine.upload(X), m)  # the handle stays usable, under the solver it has
    assert not status.any() and st["krylov_iterations"] > 0 and st["factorizations"] == 0
    _converged_sweep_check("refusals/still-usable", coeffs, Z, W, X, engine.download(dQ, m), 1e-10)
