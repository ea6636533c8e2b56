"""Eigenvalue-count estimate of polynomial and term handles on the device (feasthip_poly_estimate_count: k_node_combine,
k_spmm_fanin_trace) and the fpm[14] = 2 / M0 = "auto" modes of feast_polynomial and feast_nonlinear built on it.

Every sample is compared with the numpy restatement (count_reference.samples) on the block V the call returns.  The tolerance is
that of the pencil estimate's samples (tests/test_gpu_estimate.py), 1e-9 max(|t|, 1), with the condition bound of the
neighbouring sweep tests (tests/test_gpu_polynomial_sparse.py), 1e3 EPS cond, in place of 1e-9 where that is larger; cond is the
largest condition number of the T(z_e)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import count_reference as cr
import feastkit_jl_amd as fk
import nonlinear_cases as nc
import nonlinear_reference as nr
import polynomial_cases as pc
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd import hip_backend as hb
from feastkit_jl_amd.ingest import polynomial_union_csr
from feastkit_jl_amd.types import FeastHipError
from test_estimate import rademacher

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SEED = 20260515
M0_ERROR, INTERNAL_ERROR, FPM_ERROR = 2, 7, 9


def _tol(h, cond):
    return max(1e-9, 1e3 * EPS * cond) * np.maximum(np.abs(h), 1.0)


def contour(center, radius, ne=16, trapezoid=False):
    fpm = fk.feastinit()
    fpm[8] = ne
    if trapezoid:
        fpm[16] = 1
    return fk.feast_gcontour(center, radius, fk.feastdefault(fpm))


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")


def _setup(engine, mats, funcs, Z, W, sparse, solver="direct", **solver_kw):
    """the handle of the drivers' _poly_setup -> (F, G) of the restatement; the device's G comes from the package's own tables"""
    engine.set_adjoint(False)
    terms = funcs is not None
    if sparse:
        engine.set_polynomial_csr(*polynomial_union_csr(list(mats)), terms=terms)
    else:
        engine.set_polynomial(cr.dense(mats), terms=terms)
    if solver == "direct":
        engine.set_solver("direct", cache_factors=True, factor_precision=64)
    else:
        engine.set_solver(solver, atol=0.0, factor_precision=64, **solver_kw)
    engine.set_real_projection(False)
    engine.set_contour(Z, W, 1.0)
    if terms:
        F, G = cr.term_tables(funcs, Z, W)
        engine.nep_set_node_values(hb.nep_table(hb.nep_functions(funcs), Z))
        return F, G, W[:, None] * hb.nep_derivative_table(hb.nep_functions(funcs), Z)
    F, G = cr.poly_tables(len(mats) - 1, Z, W)
    return F, G, W[:, None] * hb.poly_derivative_table(len(mats) - 1, Z)


def _check_samples(engine, mats, F, G, Gdev, m, seed, label, kept=None):
    """one call against the restatement on the returned block; the call again: the same bits -> (t, reference t)"""
    N = mats[0].shape[0]
    t, status, st, dV = engine.poly_estimate_count(m, seed, Gdev, want_block=True)
    V = engine.download(dV, m)
    assert V.shape == (N, m) and np.all(V.imag == 0.0)
    assert np.array_equal(V.real, rademacher(seed, np.arange(N), np.arange(m)))
    h, cond = cr.samples(mats, F, G, V.real)
    err = np.abs(t - h)
    print("%s: N %d m %d ne %d cond %.2e mean %.3f%+.3fi largest error %.2e bound %.2e" % (
        label, N, m, len(F), cond, np.mean(t).real, np.mean(t).imag, err.max(), _tol(h, cond).min()))
    assert not status.any()
    assert np.all(err <= _tol(h, cond))
    if kept is not None:
        assert int(np.count_nonzero(np.abs(Gdev).max(axis=0))) == kept
    t2, status2, st2 = engine.poly_estimate_count(m, seed, Gdev)
    assert np.array_equal(t, t2) and not status2.any()
    return t, h, st, st2


# ---- samples against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,m", [(70, 2, 12), (45, 8, 15), (193, 2, 72)])
def test_samples_dense_polynomial(engine, restore, N, d, m):
    """(45, 8, 15): eight kept terms; (193, 2, 72): two panels, 64 + 8 columns"""
    mats = pc.random_coeffs(N, d, True)
    Z, W = contour(pc.CENTER, pc.RADIUS)
    F, G, Gdev = _setup(engine, mats, None, Z, W, False)
    _, _, st, st2 = _check_samples(engine, mats, F, G, Gdev, m, SEED + N, "dense polynomial d %d" % d, kept=d)
    assert st["factorizations"] == 16 and st2["factorizations"] == 0


def _middle_constant(terms):
    """random_terms(., 3, .) with its constant function moved to the middle: the dropped term sits between two kept ones"""
    return [terms[1], terms[0], terms[2]]


TERM_CASES = [(2, False, False), (2, True, False), (3, False, False), (3, True, True), (9, False, False), (9, True, False)]


@pytest.mark.parametrize("nterms,cplx,middle", TERM_CASES, ids=["nt%d-%s%s" % (n, "complex" if c else "real", "-constant-in-the-middle" if mid else "")
                                                                for n, c, mid in TERM_CASES])
def test_samples_dense_terms(engine, restore, nterms, cplx, middle):
    N, m = 45, 15
    terms = nc.random_terms(N, nterms, cplx)
    if middle:
        terms = _middle_constant(terms)
    mats, funcs = [t[0] for t in terms], [t[1] for t in terms]
    Z, W = contour(0.1 - 0.2j, 0.9)
    F, G, Gdev = _setup(engine, mats, funcs, Z, W, False)
    if middle:
        assert np.all(Gdev[:, 1] == 0.0) and np.abs(Gdev[:, 0]).min() > 0 and np.abs(Gdev[:, 2]).min() > 0
    _check_samples(engine, mats, F, G, Gdev, m, SEED + nterms, "dense terms nt %d" % nterms, kept=nterms - 1)


@functools.lru_cache(maxsize=None)
def _sparse_case(grid, d, cplx):
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    return coeffs, sc.dense(coeffs)


@pytest.mark.parametrize("m", [5, 16, 40])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("d", [1, 2, 8])
@pytest.mark.parametrize("grid", sc.GRIDS, ids=["N63", "N286", "N320"])
def test_samples_sparse_polynomial(engine, restore, grid, d, cplx, m):
    """panel widths 16 (m = 5, 16) and 64 (m = 40); d = 8 with its coefficient without entries: the full fan-in"""
    coeffs, dense = _sparse_case(grid, d, cplx)
    Z, W = contour(*sc.sweep_circle(grid))
    F, G, Gdev = _setup(engine, coeffs, None, Z, W, True)
    _check_samples(engine, dense, F, G, Gdev, m, SEED + d, "sparse d %d %s" % (d, "complex" if cplx else "real"), kept=d)


def test_samples_sparse_terms(engine, restore):
    """a term handle on CSR matrices (the grid delay problem): one constant term, width 32"""
    case = nc.grid_delay_case((6, 5, 4))
    mats, funcs = [t[0] for t in case["terms"]], [t[1] for t in case["terms"]]
    Z, W = contour(case["center"], case["radius"])
    F, G, Gdev = _setup(engine, mats, funcs, Z, W, True)
    _check_samples(engine, cr.dense(mats), F, G, Gdev, 24, SEED, "sparse terms", kept=2)


@pytest.mark.parametrize("ne,sparse", [(5, True), (5, False), (70, True), (70, False)], ids=["trapezoid5-sparse", "trapezoid5-dense", "trapezoid70-sparse",
                                                                                             "trapezoid70-dense"])
def test_samples_other_contours(engine, restore, ne, sparse):
    """an odd node count, and more nodes than a wavefront has lanes; width 32"""
    grid = sc.GRIDS[0]
    coeffs, dense = _sparse_case(grid, 2, True)
    Z, W = contour(*sc.sweep_circle(grid), ne=ne, trapezoid=True)
    assert len(Z) == ne
    F, G, Gdev = _setup(engine, coeffs if sparse else dense, None, Z, W, sparse)
    _, _, st, _ = _check_samples(engine, dense, F, G, Gdev, 24, SEED, "trapezoid %d" % ne, kept=2)
    assert st["factorizations"] == ne


def test_sparse_and_dense_handles_agree(engine, restore):
    grid = sc.GRIDS[1]
    coeffs, dense = _sparse_case(grid, 2, True)
    Z, W = contour(*sc.sweep_circle(grid))
    m = 40
    F, G, Gdev = _setup(engine, coeffs, None, Z, W, True)
    ts, status, _ = engine.poly_estimate_count(m, SEED, Gdev)
    _setup(engine, dense, None, Z, W, False)
    td, status_d, _ = engine.poly_estimate_count(m, SEED, Gdev)
    h, cond = cr.samples(dense, F, G, rademacher(SEED, np.arange(dense[0].shape[0]), np.arange(m)))
    print("sparse_direct against the dense expansion: %.2e (bound %.2e)" % (np.abs(ts - td).max(), _tol(h, cond).min()))
    assert not status.any() and not status_d.any()
    assert np.all(np.abs(ts - td) <= _tol(h, cond))


# ---- Krylov solvers -------------------------------------------------------------------------------------------------------------------
def _symmetric_coeffs(grid):
    """L + 4 I - lambda I + 1e-4 lambda^2 L: every coefficient exactly symmetric, the spectrum within 2e-3 of that of L + 4 I"""
    L = sc.laplacian(*grid)
    I = sp.identity(L.shape[0], format="csr")
    return [sp.csr_matrix(L + 4.0 * I), sp.csr_matrix(-I), sp.csr_matrix(1e-4 * L)]


@pytest.mark.parametrize("solver", ["bicgstab", "gmres", "cocg"])
def test_krylov_samples_agree_with_direct(engine, restore, solver):
    grid = sc.GRIDS[0]
    coeffs = _symmetric_coeffs(grid) if solver == "cocg" else list(_sparse_case(grid, 2, True)[0])
    Z, W = contour(*sc.sweep_circle(grid))
    m = 16
    _, _, Gdev = _setup(engine, coeffs, None, Z, W, True)
    td, status_d, _ = engine.poly_estimate_count(m, SEED, Gdev)
    _setup(engine, coeffs, None, Z, W, True, solver, rtol=1e-10, maxit=2000, restart=30)
    tk, status_k, st = engine.poly_estimate_count(m, SEED, Gdev)
    err = np.abs(tk - td)
    print("%s: iterations %d products %d largest difference from the direct samples %.2e" % (solver, st["krylov_iterations"], st["spmm_calls"], err.max()))
    assert not status_d.any() and not status_k.any()
    assert st["factorizations"] == 0 and st["krylov_iterations"] > 0 and st["spmm_calls"] > 0
    assert engine.last_node_iterations(16).min() > 0
    assert np.all(err <= 1e-6 * np.maximum(np.abs(td), 1.0))


# ---- the factor cache -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [True, False], ids=["sparse", "dense"])
def test_factor_cache_is_shared_with_the_sweeps(engine, restore, sparse):
    grid = sc.GRIDS[0]
    coeffs, dense = _sparse_case(grid, 2, False)
    Z, W = contour(*sc.sweep_circle(grid))
    m = 8
    X = engine.upload(sc.random_block(dense[0].shape[0], m, 3))
    _, _, Gdev = _setup(engine, coeffs if sparse else dense, None, Z, W, sparse)
    _, _, st = engine.poly_estimate_count(m, SEED, Gdev)
    _, status, sw = engine.poly_resinv_apply(X, m)
    assert st["factorizations"] == 16 and sw["factorizations"] == 0 and not status.any()
    _setup(engine, coeffs if sparse else dense, None, Z, W, sparse)          # a new problem: the cache is empty again
    _, status, sw = engine.poly_resinv_apply(X, m)
    _, _, st = engine.poly_estimate_count(m, SEED, Gdev)
    assert sw["factorizations"] == 16 and st["factorizations"] == 0 and not status.any()


# ---- refusals of the ABI ----------------------------------------------------------------------------------------------------------------
def _raw(engine, m, G, samples=True, seed=1):
    Gc = None if G is None else np.ascontiguousarray(G, dtype=np.complex128)
    out = np.zeros(2 * max(1, m)) if samples else None
    status = np.zeros(max(1, engine.ne), dtype=np.int32)
    rc = engine.lib.feasthip_poly_estimate_count(engine.h, m, C.c_uint64(seed), None if Gc is None else Gc.ctypes.data_as(C.c_void_p),
                                                 None if out is None else out.ctypes.data_as(C.POINTER(C.c_double)), None,
                                                 status.ctypes.data_as(C.c_void_p), None)
    return rc, engine.lib.feasthip_last_error(engine.h).decode()


def test_abi_refusals(engine, restore):
    N, d, m = 45, 3, 5
    mats = pc.random_coeffs(N, d, True)
    Z, W = contour(pc.CENTER, pc.RADIUS)
    _, _, Gdev = _setup(engine, mats, None, Z, W, False)
    assert _raw(engine, m, Gdev)[0] == 0
    assert _raw(engine, m, None)[0] == INTERNAL_ERROR and _raw(engine, m, Gdev, samples=False)[0] == INTERNAL_ERROR
    assert engine.lib.feasthip_poly_estimate_count(None, m, C.c_uint64(1), None, None, None, None, None) == INTERNAL_ERROR
    for bad in (0, -3, N + 1):
        assert _raw(engine, bad, Gdev)[0] == M0_ERROR
    for value in (np.nan, np.inf * 1j):
        Gbad = Gdev.copy()
        Gbad[11, 2] = value
        rc, msg = _raw(engine, m, Gbad)
        assert rc == FPM_ERROR and "node 11" in msg and "term 2" in msg
    with pytest.raises(ValueError):
        engine.poly_estimate_count(m, 1, Gdev[:, :3])
    # the pencil estimate and its block stay closed to a polynomial handle
    for call in (lambda: engine.estimate_count(m, 1), lambda: engine.random_block(m, 1)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "feasthip_poly_" in str(err.value)
    # a term handle without node values, and with values of another contour
    terms = nc.random_terms(N, 3, True)
    funcs = hb.nep_functions([t[1] for t in terms])
    engine.set_polynomial([t[0] for t in terms], terms=True)
    engine.set_contour(Z, W, 1.0)
    Gt = W[:, None] * hb.nep_derivative_table(funcs, Z)
    rc, msg = _raw(engine, m, Gt)
    assert rc == FPM_ERROR and "feasthip_nep_set_node_values" in msg
    engine.nep_set_node_values(hb.nep_table(funcs, Z))
    assert _raw(engine, m, Gt)[0] == 0
    Z2, W2 = contour(pc.CENTER, 0.5 * pc.RADIUS)
    engine.set_contour(Z2, W2, 1.0)
    assert _raw(engine, m, Gt)[0] == FPM_ERROR
    # a dense and a CSR pencil handle
    T = np.diag(np.arange(1.0, 9.0))
    for A in (T, sp.csr_matrix(T)):
        engine.set_problem(A)
        engine.set_contour(Z, W, 1.0)
        engine.poly_degree = 1
        with pytest.raises(FeastHipError) as err:
            engine.poly_estimate_count(2, 1, np.ones((16, 2)))
        assert err.value.code == FPM_ERROR and "feasthip_set_polynomial" in str(err.value)
    res = fk.feast_general(T, None, 2.5, 1.0, M0=4, engine=engine)          # and the engine is an ordinary one again
    assert res.info == 0 and res.M == 2


# ---- the drivers: fpm[14] = 2 -----------------------------------------------------------------------------------------------------------
def _fpm(fpm3=10, ne=16, estimate=False):
    fpm = fk.feastinit()
    fpm[8], fpm[3] = ne, fpm3
    if estimate:
        fpm[14] = 2
    return fpm


def _restated(mats, funcs, center, radius, m, seed, ne=16):
    """(mean, stderr, samples) of the restatement for the Rademacher block of `seed`"""
    Z, W = contour(center, radius, ne)
    F, G = cr.poly_tables(len(mats) - 1, Z, W) if funcs is None else cr.term_tables(funcs, Z, W)
    t, _ = cr.samples(mats, F, G, rademacher(seed, np.arange(mats[0].shape[0]), np.arange(m)))
    return cr.mean_stderr(t) + (t,)


def _check_estimate(res, mats, funcs, center, radius, m, seed, solver, dropped):
    mean, stderr, _ = _restated(cr.dense(mats), funcs, center, radius, m, seed)
    est = res.stats["estimate"]
    print("estimate %.4f%+.4fi +- %.3f (restatement %.4f%+.4fi +- %.3f), M %d, %.3f s" % (
        est["mean"].real, est["mean"].imag, est["stderr"], mean.real, mean.imag, stderr, res.M, est["seconds"]))
    assert res.info == 0 and res.M == cr.count(mean)
    assert abs(est["mean"] - mean) <= 1e-8 and abs(est["stderr"] - stderr) <= 1e-8
    assert res.lambda_.shape == (0,) and res.q.shape == (mats[0].shape[0], 0) and res.res.shape == (0,)
    assert np.iscomplexobj(res.lambda_) and np.iscomplexobj(res.q) and res.loop == 0
    assert est["nodes"] == 16 and est["solver"] == solver and est["seed"] == seed and len(est["samples"]) == m
    assert est["dropped_terms"] == dropped and est["seconds"] > 0


@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_estimate_driver_dense_polynomial(engine, restore, params):
    N, d, k, _, monic = params
    case = pc.make_case(N, d, k, monic)
    for method in ("linearised", "projected"):          # validated, and the estimate is the same
        res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=32, fpm=_fpm(estimate=True), engine=engine, seed=7, method=method)
        _check_estimate(res, case["coeffs"], None, case["center"], case["radius"], 32, 7, "direct", [0])


@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES, ids=sc.DRIVER_IDS)
def test_estimate_driver_damped(engine, restore, name, scaled):
    case = sc.damped_case(name, scaled)
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=64, fpm=_fpm(estimate=True), engine=engine, solver="sparse_direct",
                              method="projected")
    _check_estimate(res, case["coeffs"], None, case["center"], case["radius"], 64, SEED, "sparse_direct", [0])
    assert "solver_substitution" not in res.stats


def test_estimate_driver_nonlinear(engine, restore):
    case = nc.rational_case()
    mats, funcs = [t[0] for t in case["terms"]], [t[1] for t in case["terms"]]
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=40, fpm=_fpm(estimate=True), engine=engine, seed=3)
    _check_estimate(res, mats, funcs, case["center"], case["radius"], 40, 3, "direct", [0])
    case = nc.grid_delay_case((6, 5, 4))
    mats, funcs = [t[0] for t in case["terms"]], [t[1] for t in case["terms"]]
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=48, fpm=_fpm(estimate=True), engine=engine, solver="sparse_direct")
    _check_estimate(res, mats, funcs, case["center"], case["radius"], 48, SEED, "sparse_direct", [0])


def test_estimate_driver_krylov_and_a_failed_node(engine, restore):
    case = sc.damped_case("20x16", False)
    args = (list(case["coeffs"]), case["center"], case["radius"])
    direct = fk.feast_polynomial(*args, M0=16, fpm=_fpm(estimate=True), engine=engine, solver="sparse_direct", method="projected")
    res = fk.feast_polynomial(*args, M0=16, fpm=_fpm(estimate=True), engine=engine, solver="bicgstab", method="projected", solver_maxiter=4000)
    est = res.stats["estimate"]
    print("bicgstab estimate %.4f against direct %.4f" % (est["mean"].real, direct.stats["estimate"]["mean"].real))
    assert res.info == 0 and est["solver"] == "bicgstab" and est["solver_tol"] == fk.api.ESTIMATE_TOL
    assert abs(est["mean"] - direct.stats["estimate"]["mean"]) <= 1e-5
    # the estimate has one right-hand-side block for all nodes, so the Krylov names pass under the default method too
    lin = fk.feast_polynomial(*args, M0=16, fpm=_fpm(estimate=True), engine=engine, solver="bicgstab", solver_maxiter=4000)
    assert lin.info == 0 and np.array_equal(lin.stats["estimate"]["samples"], est["samples"])
    with pytest.raises(ValueError, match="projected"):
        fk.feast_polynomial(*args, M0=4, fpm=_fpm(), engine=engine, solver="bicgstab")
    capped = fk.feast_polynomial(*args, M0=16, fpm=_fpm(estimate=True), engine=engine, solver="bicgstab", method="projected", solver_maxiter=2)
    assert capped.info == int(fk.FeastError.Feast_ERROR_NO_CONVERGENCE) and capped.stats["estimate"] is None and capped.M == 0


# ---- the drivers: M0 = "auto" -----------------------------------------------------------------------------------------------------------
def _auto_rule(mats, funcs, center, radius, seed, d=None):
    N = mats[0].shape[0]
    mean, stderr, _ = _restated(cr.dense(mats), funcs, center, radius, min(64, N), seed)          # (an estimate takes at most N columns)
    return (cr.auto_M0(mean, stderr, N) if d is None else cr.auto_M0_linearised(mean, stderr, N, d)), mean, stderr


def _check_auto(res, M0a, mean, stderr):
    est = res.stats["estimate"]
    samples = min(64, res.q.shape[0])
    print("M0 = auto: %d (estimate %.3f +- %.3f), loop %d, M %d, factorizations %d" % (res.stats["M0_auto"], est["mean"].real, est["stderr"], res.loop, res.M,
                                                                                     res.stats["factorizations"]))
    assert res.stats["M0_auto"] == M0a
    assert abs(est["mean"] - mean) <= 1e-8 and abs(est["stderr"] - stderr) <= 1e-8 and len(est["samples"]) == samples and est["nodes"] == 16
    assert res.stats["factorizations"] == 16


def test_auto_projected_sparse_direct(engine, restore):
    case = sc.damped_case("20x16", False)
    M0a, mean, stderr = _auto_rule(case["coeffs"], None, case["center"], case["radius"], SEED)
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0="auto", fpm=_fpm(sc.FPM3, sc.NE), engine=engine,
                              solver="sparse_direct", method="projected")
    _check_auto(res, M0a, mean, stderr)
    poly = res.stats["polynomial"]
    lam_err = pr.match_error(res.lambda_, case["lam_in"]) if res.M == len(case["lam_in"]) else np.inf
    print("eigenvalue error %.2e history %s" % (lam_err, ["%.1e" % e for e in poly["eps_history"]]))
    assert res.info == 0 and res.M == len(case["lam_in"]) and poly["columns"] == M0a and poly["plan"] == "multifrontal" and poly["fell_back"] is False
    assert lam_err <= 1e-8          # (test_gpu_polynomial_projected.py: _check_result)


def test_auto_linearised_dense(engine, restore):
    N, d, k, _, monic = pc.DRIVER_CASES[0]
    case = pc.make_case(N, d, k, monic)
    M0a, mean, stderr = _auto_rule(case["coeffs"], None, case["center"], case["radius"], SEED, d)
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0="auto", fpm=_fpm(pc.FPM3, pc.NE), engine=engine)
    _check_auto(res, M0a, mean, stderr)
    lam_err = pr.match_error(res.lambda_, case["lam_in"]) if res.M == k else np.inf
    print("eigenvalue error %.2e history %s" % (lam_err, ["%.1e" % e for e in res.stats["polynomial"]["eps_history"]]))
    assert res.info == 0 and res.M == k and res.stats["polynomial"]["columns"] == M0a * d
    assert lam_err <= 1e-9          # (test_gpu_polynomial.py: test_driver)


@pytest.mark.parametrize("which", ["rational", "grid-6x5x4"])
def test_auto_nonlinear(engine, restore, which):
    case = nc.rational_case() if which == "rational" else nc.grid_delay_case((6, 5, 4))
    solver = "direct" if which == "rational" else "sparse_direct"
    mats, funcs = [t[0] for t in case["terms"]], [t[1] for t in case["terms"]]
    M0a, mean, stderr = _auto_rule(mats, funcs, case["center"], case["radius"], 1)
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0="auto", fpm=_fpm(nc.FPM3, nc.NE), engine=engine, solver=solver, seed=1)
    _check_auto(res, M0a, mean, stderr)
    # the bound of test_gpu_nonlinear.py (_check): ten times the error of the restatement's run from the same start block
    ref = nr.driver(case["terms"], case["center"], case["radius"], M0a, seed=1)
    ref_err = nr.match_error(ref["lam"], case["lam_in"]) if ref["M"] == case["count"] else np.inf
    lam_err = nr.match_error(res.lambda_, case["lam_in"]) if res.M == case["count"] else np.inf
    print("eigenvalue error %.2e (restatement %.2e) history %s" % (lam_err, ref_err, ["%.1e" % e for e in res.stats["nonlinear"]["eps_history"]]))
    assert res.info == 0 and res.M == case["count"] and res.stats["nonlinear"]["columns"] == M0a
    assert lam_err <= max(10 * ref_err, 1e-12)
