"""feast_polynomial(..., solver="sparse_direct") on the device: the feasthip_poly_* primitives on a sparse polynomial handle
(multifrontal LU of P(z_e) through k_mf_assemble_poly, fan-out products through k_spmm_fan) against numpy on the densified
coefficients and on the explicit companion, against the dense polynomial handle and (degree 1) the CSR pencil, the factor
cache, the driver on the analytic damped cases pinned by tests/test_polynomial_sparse_host.py, the dense fallback, and the
refusals of the ABI.  Bounds and assertion forms are those of tests/test_gpu_polynomial.py for the same quantities."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import feast_oracle as fo
import feastkit_jl_amd as fk
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd.ingest import polynomial_union_csr
from feastkit_jl_amd.types import FeastHipError

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FPM_ERROR = 9
MF = 2               # engine.band_plan()[3] of the multifrontal plan


def _contour(ne, grid=None):
    """the circle of the solve and product tests, on which P(z) is diagonally dominant; with a grid, the circle of the sweep
    tests, which has eigenvalues inside (a contour sum with none inside is zero up to the quadrature error)"""
    center, radius = (sc.CENTER, sc.RADIUS) if grid is None else sc.sweep_circle(grid)
    return fo.feast_gcontour(center, radius, ne)


def _setup(engine, coeffs, ne=sc.NE, grid=None):
    engine.set_adjoint(False)
    engine.set_polynomial_csr(*polynomial_union_csr(coeffs))
    engine.set_solver("direct", cache_factors=True, factor_precision=64)
    engine.set_real_projection(False)
    Zne, Wne = _contour(ne, grid)
    engine.set_contour(Zne, Wne, 1.0)
    return Zne, Wne


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")


@pytest.fixture(params=["8", "64"])
def leaf(request, monkeypatch):
    """FH_MF_LEAF: at 8 the elimination tree has several levels even at N = 63"""
    monkeypatch.setenv("FH_MF_LEAF", request.param)
    return int(request.param)


# (grid, d, complex coefficients)
SOLVE_SHAPES = [((9, 7, 1), 1, True), ((9, 7, 1), 4, False), ((13, 11, 2), 2, True), ((13, 11, 2), 3, False), ((20, 16, 1), 1, False), ((20, 16, 1), 3, True),
                ((9, 7, 1), 8, True)]
# (grid, d, m, complex coefficients): d = 1 .. 4 and 8 (the degree bound: full fan width), m = 5, 64, 72 (two panels), every N
SWEEP_SHAPES = [((9, 7, 1), 1, 5, False), ((9, 7, 1), 4, 5, True), ((9, 7, 1), 3, 72, False), ((13, 11, 2), 2, 72, False), ((20, 16, 1), 2, 64, True),
                ((9, 7, 1), 8, 5, True)]
# (the d = 8 row goes last here too: pytest numbers the grids by position, and the ids of the other rows stay as they were)
PRODUCT_SHAPES = SWEEP_SHAPES[:5] + [((13, 11, 2), 4, 64, True), ((20, 16, 1), 3, 72, False)] + SWEEP_SHAPES[5:]


@pytest.mark.parametrize("m", [5, 64])
@pytest.mark.parametrize("grid,d,cplx", SOLVE_SHAPES)
def test_poly_solve(engine, restore, leaf, grid, d, cplx, m):
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    dense = sc.dense(coeffs)
    N = dense[0].shape[0]
    Zne, _ = _setup(engine, coeffs)
    z = Zne[3]
    R = sc.random_block(N, m, 11)
    dY, rc = engine.poly_solve(z, engine.upload(R), m)
    Y = engine.download(dY, m)
    assert engine.band_plan()[3] == MF
    P = pr.poly_at(dense, z)
    berr = np.linalg.norm(P @ Y - R) / (np.linalg.norm(P) * np.linalg.norm(Y) + np.linalg.norm(R))
    print("N %d d %d m %d leaf %d backward error %.2e bound %.2e" % (N, d, m, leaf, berr, 64 * N * EPS))
    assert rc == 0
    assert berr <= 64 * N * EPS
    if d == 1:
        # the same solve on the CSR pencil (-A_0, A_1): z A_1 - (-A_0) = P(z); Horner and z B - A round differently
        engine.set_problem(sp.csr_matrix(-coeffs[0]), sp.csr_matrix(coeffs[1]))
        engine.set_solver("banded", cache_factors=True, factor_precision=64)
        mm = min(m, N)                      # (a pencil handle takes at most N columns; poly_solve takes any count)
        dY2, rc2 = engine.shifted_solve(z, engine.upload(np.asfortranarray(R[:, :mm])), mm)
        Y2 = engine.download(dY2, mm)
        cond = np.linalg.cond(P)
        diff = np.linalg.norm(Y[:, :mm] - Y2) / np.linalg.norm(Y2)
        print("against shifted_solve on (-A_0, A_1): %.2e, cond %.2e" % (diff, cond))
        assert rc2 == 0 and diff <= 64 * N * EPS * cond


@functools.lru_cache(maxsize=None)
def _sweep_reference(grid, d, m, cplx, ne):
    """contour sum on the explicit companion (numpy.linalg.solve per node), computed once per shape"""
    dense = sc.dense(sc.mixed_pattern_coeffs(grid, d, cplx))
    Zne, Wne = _contour(ne, grid)
    Q = sc.random_block(d * dense[0].shape[0], m, 13)
    ref, conds = pr.contour_sum(dense, Zne, Wne, Q)
    return Q, ref, float(conds.max())


@pytest.mark.parametrize("ne", [8, 16])
@pytest.mark.parametrize("grid,d,m,cplx", SWEEP_SHAPES)
def test_poly_contour_apply(engine, restore, grid, d, m, cplx, ne):
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    N = coeffs[0].shape[0]
    Q, ref, cond = _sweep_reference(grid, d, m, cplx, ne)
    _setup(engine, coeffs, ne, grid)
    dP, status, st = engine.poly_contour_apply(engine.upload(Q), m)
    P = engine.download(dP, m)
    err = np.linalg.norm(P - ref) / np.linalg.norm(ref)
    print("N %d d %d m %d ne %d: cond max %.2e, relative error %.2e, bound %.2e" % (N, d, m, ne, cond, err, 1e3 * EPS * cond))
    assert not status[:ne].any() and st["factorizations"] == ne
    assert P.shape == (d * N, m)
    assert err <= 1e3 * EPS * cond
    # the dense polynomial handle on the same coefficients: the two flavours agree to the sweep bound
    engine.set_polynomial(sc.dense(coeffs))
    dD, status, _ = engine.poly_contour_apply(engine.upload(Q), m)
    D = engine.download(dD, m)
    diff = np.linalg.norm(P - D) / np.linalg.norm(D)
    print("sparse against dense handle: %.2e" % diff)
    assert not status[:ne].any() and diff <= 1e3 * EPS * cond


def test_poly_contour_apply_small_leaves(engine, restore, leaf):
    grid, d, m, cplx = SWEEP_SHAPES[3]
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    Q, ref, cond = _sweep_reference(grid, d, m, cplx, 8)
    _setup(engine, coeffs, 8, grid)
    dP, status, st = engine.poly_contour_apply(engine.upload(Q), m)
    err = np.linalg.norm(engine.download(dP, m) - ref) / np.linalg.norm(ref)
    print("leaf %d: relative error %.2e, bound %.2e" % (leaf, err, 1e3 * EPS * cond))
    assert not status[:8].any() and st["factorizations"] == 8 and err <= 1e3 * EPS * cond


@pytest.mark.parametrize("grid,d,m,cplx", PRODUCT_SHAPES)
def test_products_projection_residual(engine, restore, grid, d, m, cplx):
    """d >= 3 runs k_spmm_fan with 1, 2, .. d + 1 outputs, accumulating and not"""
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    dense = sc.dense(coeffs)
    N = dense[0].shape[0]
    _setup(engine, coeffs)
    A, B = pr.companion(dense)
    nA, nB = np.linalg.norm(A), np.linalg.norm(B)
    unit = 16 * d * N * EPS
    X = sc.random_block(d * N, m, 17)
    dX = engine.upload(X)
    for which, op, nop in ((0, A, nA), (1, B, min(nA, nB))):
        Y = engine.download(engine.poly_matmul(which, dX, m), m)
        err = np.linalg.norm(Y - op @ X)
        print("matmul %d: error %.2e bound %.2e" % (which, err, unit * nop * np.linalg.norm(X)))
        assert err <= unit * nop * np.linalg.norm(X)
    Aq, Sq = engine.poly_project(dX, m)
    for name, G, op in (("Aq", Aq, A), ("Sq", Sq, B)):
        err = np.linalg.norm(G - X.conj().T @ (op @ X))
        print("%s: error %.2e bound %.2e" % (name, err, unit * nA * np.linalg.norm(X) ** 2))
        assert err <= unit * nA * np.linalg.norm(X) ** 2
    rng = np.random.default_rng(19)
    V = np.asfortranarray(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))
    lam = sc.CENTER + 0.7 * (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m))
    M = m - 3
    Xr = X @ V
    nrm = np.linalg.norm(Xr, axis=0)
    Xr[:, :M] /= nrm[:M]
    bwd_ref = pr.backward_error(dense, lam[:M], Xr[:N, :M])
    for use_B in (True, False):
        dXg, res, bwd = engine.poly_ritz_residual(dX, m, V, lam, M, normalize=True, use_B=use_B)
        Xg = engine.download(dXg, m)
        xerr = np.abs(Xg - Xr).max()
        xbound = unit * np.linalg.norm(X) * np.linalg.norm(V) / nrm.min()
        BX = B @ Xr if use_B else Xr
        res_ref = np.array([np.linalg.norm(A @ Xr[:, j] - lam[j] * BX[:, j]) / max(abs(lam[j]), 1.0) for j in range(M)])
        print("use_B %d: X error %.2e (bound %.2e), residual error %.2e (bound %.2e), backward error difference %.2e (bound %.2e)" % (
            use_B, xerr, xbound, np.abs(res - res_ref).max(), unit * nA, np.abs(bwd - bwd_ref).max(), unit))
        assert xerr <= xbound
        assert len(res) == M and np.abs(res - res_ref).max() <= unit * nA
        assert len(bwd) == M and np.abs(bwd - bwd_ref).max() <= unit


def test_factor_cache(engine, restore):
    grid, d, m = (13, 11, 2), 2, 12
    coeffs = sc.mixed_pattern_coeffs(grid, d, True)
    N = coeffs[0].shape[0]
    _setup(engine, coeffs)
    dQ = engine.upload(sc.random_block(d * N, m, 23))
    dP1, _, st1 = engine.poly_contour_apply(dQ, m)
    dP2, _, st2 = engine.poly_contour_apply(dQ, m)
    assert st1["factorizations"] == sc.NE and st2["factorizations"] == 0
    assert np.array_equal(engine.download(dP1, m), engine.download(dP2, m))
    # the plan is described by the calls the sparse direct solver has
    factor_bytes, transient_bytes = engine.direct_plan_bytes(sc.NE)
    assert engine.band_plan()[3] == MF and engine.direct_plan_flops() > 0 and factor_bytes > 0 and transient_bytes > 0
    engine.free_factors()
    _, _, st3 = engine.poly_contour_apply(dQ, m)
    assert st3["factorizations"] == sc.NE


def _fpm():
    fpm = fk.feastinit()
    fpm[8], fpm[3] = sc.NE, sc.FPM3
    return fpm


@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES, ids=sc.DRIVER_IDS)
def test_driver(engine, restore, name, scaled):
    """The two cases pinned on the restatement by tests/test_polynomial_sparse_host.py (seed 20260515): 20 x 16 monic real stops at
    loop 4 (5.5e-10 at loop 3, 3.3e-12 at loop 4), 24 x 18 scaled complex at loop 5 (1.0e-9, 1.9e-11)."""
    case = sc.damped_case(name, scaled)
    N, k, M0 = case["N"], case["k"], case["M0"]
    dense = sc.dense(case["coeffs"])
    Q0 = fo.seeded_subspace(2 * N, 2 * M0, 20260515)
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=M0, fpm=_fpm(), engine=engine, Q0=Q0,
                              solver="sparse_direct")
    poly = res.stats["polynomial"]
    lam_err = pr.match_error(res.lambda_, case["lam_in"])
    bwd_np = pr.backward_error(dense, res.lambda_, res.q)
    print("loop %d (restatement %d) epsout %.2e history %s eigenvalue error %.2e backward error %.2e (numpy on q: %.2e) factorizations %d" % (
        res.loop, case["loop"], res.epsout, ["%.1e" % e for e in poly["eps_history"]], lam_err, poly["backward_error"].max(), bwd_np.max(),
        res.stats["factorizations"]))
    print("plan %s: %d factor bytes and %.3e flop per node, nnz %d" % (poly["plan"], poly["plan_factor_bytes"], poly["plan_flops"], poly["plan_nnz"]))
    assert res.info == 0 and res.M == k == 5
    assert res.loop == case["loop"]
    assert res.epsout <= 1e-10
    assert lam_err <= 1e-9
    assert poly["backward_error"].max() <= 1e-11
    assert res.q.shape == (N, k)
    assert np.abs(bwd_np - poly["backward_error"]).max() <= 16 * 2 * N * EPS
    assert poly["degree"] == 2 and poly["columns"] == 2 * M0 and len(poly["eps_history"]) == res.loop + 1
    assert poly["plan"] == "multifrontal" and poly["fell_back"] is False and "solver_substitution" not in res.stats
    assert poly["plan_nnz"] == len(polynomial_union_csr(case["coeffs"])[1]) and poly["plan_factor_bytes"] > 0 and poly["plan_flops"] > 0
    assert res.stats["factorizations"] == sc.NE


def test_fallback_to_the_dense_expansion(engine, restore, monkeypatch):
    """Every coefficient has a structurally zero pressure block: with small leaves a front's fully-summed block holds pressures
    without their velocities, the multifrontal LU rejects the pivot, and the call reruns on the dense expansion."""
    monkeypatch.setenv("FH_MF_LEAF", "8")
    case = sc.saddle_quadratic()
    M0 = 3            # the restatement stops at loop 2 (6.6e-9, then 1.8e-12)
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=M0, fpm=_fpm(), engine=engine, solver="sparse_direct")
    poly = res.stats["polynomial"]
    lam_err = pr.match_error(res.lambda_, case["lam_in"]) if res.M == len(case["lam_in"]) else np.inf
    print("M %d loop %d epsout %.2e eigenvalue error %.2e; %s" % (res.M, res.loop, res.epsout, lam_err, res.stats.get("solver_substitution")))
    assert poly["fell_back"] is True and poly["plan"] == "dense"
    assert res.stats["solver_substitution"]["requested"] == "sparse_direct" and "pivot" in res.stats["solver_substitution"]["reason"]
    assert res.info == 0 and res.M == len(case["lam_in"])
    assert res.epsout <= 1e-10 and lam_err <= 1e-9
    # beyond the dense window the same rejection is an error that names the cause and the sizes
    monkeypatch.setattr(fk.api, "POLY_DENSE_LIMIT", 100)
    with pytest.raises(FeastHipError) as err:
        fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=M0, fpm=_fpm(), engine=engine, solver="sparse_direct")
    assert err.value.code == 8 and "rejected a pivot" in str(err.value) and "N = %d" % case["N"] in str(err.value)


def test_abi_refusals(engine, restore):
    grid, d, m = (9, 7, 1), 3, 5
    coeffs = sc.mixed_pattern_coeffs(grid, d, False)
    N = coeffs[0].shape[0]
    _setup(engine, coeffs)
    dN = engine.upload(sc.random_block(N, m, 29))
    V, lam = np.eye(m, dtype=complex), np.zeros(m, dtype=complex)
    pencil_calls = [lambda: engine.contour_apply(dN, m), lambda: engine.project(dN, m), lambda: engine.matmul(0, dN, m),
                    lambda: engine.shifted_solve(0.5j, dN, m), lambda: engine.ritz_residual(dN, m, V, lam, m),
                    lambda: engine.orthonormalize(dN, m, 1e-8), lambda: engine.rayleigh_ritz(dN, m, -1.0, 1.0)]
    for call in pencil_calls:
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "feasthip_poly_" in str(err.value)
    for call in (lambda: engine.set_adjoint(True), lambda: engine.set_solver("direct", factor_precision=32), lambda: engine.set_solver("banded"),
                 lambda: engine.set_node_range(0, 4)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "polynomial" in str(err.value)
    # none of the refused settings took hold: the handle still sweeps
    dQ = engine.upload(sc.random_block(d * N, m, 31))
    _, status, _ = engine.poly_contour_apply(dQ, m)
    assert not status.any()
    # what feasthip_set_polynomial_csr enforces: monotone pointers, columns in range and strictly increasing
    rowptr, col, vals = polynomial_union_csr(coeffs)
    bad_ptr = rowptr.copy(); bad_ptr[3] = bad_ptr[4] + 1
    bad_col = col.copy(); bad_col[5] = N
    dup_col = col.copy(); dup_col[rowptr[2] + 1] = dup_col[rowptr[2]]
    for rp, cl in ((bad_ptr, col), (rowptr, bad_col), (rowptr, dup_col)):
        with pytest.raises(FeastHipError) as err:
            engine.set_polynomial_csr(rp, cl, vals)
        assert err.value.code == 1
    # a refused ingest leaves the problem that was there
    _, status, _ = engine.poly_contour_apply(dQ, m)
    assert not status.any()
