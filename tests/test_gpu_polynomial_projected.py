"""feast_polynomial(..., method="projected") on the device: the four feasthip_poly_* calls of the projected method
(k_spmm_horner / the dense products on column-scaled panels, k_poly_resinv_acc on the cached factors, the reduced projection and
the candidate evaluation) against numpy on dense and sparse polynomial handles, and the driver held to the loop counts that
tests/test_polynomial_projected_host.py pins on the numpy restatement.  Bounds are those of tests/test_gpu_polynomial.py for the
same kinds of quantity: 16 d N eps ||A|| ||X|| for products, 1e3 eps cond_2 for contour sums."""
import ctypes
import functools

import numpy as np
import pytest

import feast_oracle as fo
import feastkit_jl_amd as fk
import polynomial_cases as pc
import polynomial_projected_reference as ppr
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd import _lib
from feastkit_jl_amd.ingest import polynomial_union_csr
from feastkit_jl_amd.types import FeastHipError

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FPM_ERROR = 9
NEW_SYMBOLS = ("feasthip_poly_eval_cols_dev", "feasthip_poly_resinv_apply_dev", "feasthip_poly_project_reduced_dev",
               "feasthip_poly_ritz_eval_dev", "feasthip_poly_orthonormalize_dev")


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")
    engine.set_ortho_method("mgs")


def _setup(engine, coeffs, contour=None, sparse=False):
    """coeffs: dense arrays, or CSR matrices with sparse=True -> the dense coefficients numpy works on"""
    engine.set_adjoint(False)
    if sparse:
        engine.set_polynomial_csr(*polynomial_union_csr(coeffs))
    else:
        engine.set_polynomial(coeffs)
    engine.set_solver("direct", cache_factors=True, factor_precision=64)
    engine.set_real_projection(False)
    if contour is not None:
        engine.set_contour(contour[0], contour[1], 1.0)
    return sc.dense(coeffs) if sparse else list(coeffs)


def test_symbols_are_declared_and_exported():
    lib = fk.load_library()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


# ---- P(lambda_j) x_j -----------------------------------------------------------------------------------------------------------
# dense: (N, d, complex); sparse: (grid, d, complex) -- every grid, d = 1 .. 4, real and complex values
EVAL_DENSE = [(70, 1, True), (70, 2, True), (45, 3, False), (130, 4, True), (45, 8, True)]
EVAL_SPARSE = [((9, 7, 1), 1, False), ((9, 7, 1), 4, True), ((13, 11, 2), 2, True), ((13, 11, 2), 3, False), ((20, 16, 1), 3, True),
               ((20, 16, 1), 2, False), ((9, 7, 1), 8, True)]
EVAL_M = [5, 24, 64, 72]          # panel widths 16, 32, 64, and 64 + 16 across the 64-column panel


def _lambdas(m):
    """distinct per column, 0 and one value outside the unit circle among them"""
    j = np.arange(m)
    lam = (0.3 + 0.6 * j / m) * np.exp(2j * np.pi * j / m * 3)
    lam[0], lam[1] = 0.0, 1.7 - 0.4j
    return lam


def _check_eval(engine, dense, N, d, m):
    lam = _lambdas(m)
    X = pc.random_block(N, m, 41)
    dX = engine.upload(X)
    R = engine.download(engine.poly_eval_cols(dX, lam, m), m)
    ref = ppr.eval_cols(dense, lam, X)
    bound = 16 * d * N * EPS * sum(np.linalg.norm(Ak) * np.linalg.norm(X * np.abs(lam)[None, :] ** k) for k, Ak in enumerate(dense))
    err = np.linalg.norm(R - ref)
    print("N %d d %d m %d: error %.2e bound %.2e" % (N, d, m, err, bound))
    assert R.shape == (N, m) and err <= bound
    assert np.array_equal(R, engine.download(engine.poly_eval_cols(dX, lam, m), m))


@pytest.mark.parametrize("m", EVAL_M)
@pytest.mark.parametrize("N,d,cplx", EVAL_DENSE)
def test_poly_eval_cols_dense(engine, restore, N, d, cplx, m):
    dense = _setup(engine, pc.random_coeffs(N, d, cplx))
    _check_eval(engine, dense, N, d, m)


@pytest.mark.parametrize("m", EVAL_M)
@pytest.mark.parametrize("grid,d,cplx", EVAL_SPARSE)
def test_poly_eval_cols_sparse(engine, restore, grid, d, cplx, m):
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    dense = _setup(engine, coeffs, sparse=True)
    _check_eval(engine, dense, dense[0].shape[0], d, m)


# ---- the contour step ------------------------------------------------------------------------------------------------------------
def _dense_sweep_case(N, d):
    return pc.make_case(N, d, {70: 6, 45: 7, 193: 9}[N], False)["coeffs"]


def _shifts(center, radius, m):
    """one shift per column inside the circle, none on a node"""
    j = np.arange(m)
    return center + radius * (0.15 + 0.6 * j / m) * np.exp(2j * np.pi * (j * 0.381966 + 0.05))


@functools.lru_cache(maxsize=None)
def _sweep_reference(kind, key, d, m, ne):
    """the restatement's plain and shifted sweeps on the dense coefficients, once per shape"""
    if kind == "dense":
        dense, center, radius = _dense_sweep_case(key, d), pc.CENTER, pc.RADIUS
    else:
        dense = sc.dense(sc.mixed_pattern_coeffs(key, d, True))
        center, radius = sc.sweep_circle(key)
    Zne, Wne = fo.feast_gcontour(center, radius, ne)
    X = pc.random_block(dense[0].shape[0], m, 43)
    sigma = _shifts(center, radius, m)
    plain, conds = ppr.sweep(dense, Zne, Wne, X, None, want_cond=True)
    shifted = ppr.sweep(dense, Zne, Wne, X, sigma)
    return (Zne, Wne), X, sigma, plain, shifted, float(conds.max())


# (the sparse row stays fourth: pytest numbers its grid by position, and its id stays as it was)
_RESINV_DENSE = [("dense", N, d, m) for N, d, m in pc.SWEEP_SHAPES]
RESINV_SHAPES = _RESINV_DENSE[:3] + [("sparse", (13, 11, 2), 2, 72)] + _RESINV_DENSE[3:]


@pytest.mark.parametrize("ne", [8, 16])
@pytest.mark.parametrize("kind,key,d,m", RESINV_SHAPES)
def test_poly_resinv_apply(engine, restore, kind, key, d, m, ne):
    contour, X, sigma, plain, shifted, cond = _sweep_reference(kind, key, d, m, ne)
    if kind == "dense":
        _setup(engine, _dense_sweep_case(key, d), contour)
    else:
        _setup(engine, sc.mixed_pattern_coeffs(key, d, True), contour, sparse=True)
    dX = engine.upload(X)
    dQ, status, st1 = engine.poly_resinv_apply(dX, m)
    Q = engine.download(dQ, m)
    err = np.linalg.norm(Q - plain) / np.linalg.norm(plain)
    print("%s d %d m %d ne %d: cond max %.2e, plain sweep error %.2e, bound %.2e" % (key, d, m, ne, cond, err, 1e3 * EPS * cond))
    assert not status[:ne].any() and st1["factorizations"] == ne
    assert Q.shape == X.shape and err <= 1e3 * EPS * cond
    dS, status, st2 = engine.poly_resinv_apply(dX, m, sigma)
    S = engine.download(dS, m)
    err = np.linalg.norm(S - shifted) / np.linalg.norm(shifted)
    print("shifted sweep error %.2e" % err)
    assert not status[:ne].any() and st2["factorizations"] == 0          # the cached factors
    assert err <= 1e3 * EPS * cond
    assert np.array_equal(S, engine.download(engine.poly_resinv_apply(dX, m, sigma)[0], m))
    # a shift on a node is refused on the host, nothing is divided by zero on the device
    bad = sigma.copy()
    bad[m // 2] = contour[0][ne // 2]
    with pytest.raises(FeastHipError) as err:
        engine.poly_resinv_apply(dX, m, bad)
    assert err.value.code == FPM_ERROR and "coincides with contour node %d" % (ne // 2) in str(err.value)
    bad[m // 2] = np.nan
    with pytest.raises(FeastHipError) as err:
        engine.poly_resinv_apply(dX, m, bad)
    assert err.value.code == FPM_ERROR


# ---- the reduced polynomial and the candidates --------------------------------------------------------------------------------
REDUCED_SHAPES = [("dense", 70, 2, 7), ("dense", 45, 3, 7), ("dense", 70, 2, 64), ("dense", 193, 2, 72), ("sparse", (9, 7, 1), 3, 7),
                  ("sparse", (13, 11, 2), 2, 72), ("sparse", (9, 7, 1), 8, 7)]


@pytest.mark.parametrize("kind,key,d,r", REDUCED_SHAPES)
def test_project_reduced_and_ritz_eval(engine, restore, kind, key, d, r):
    if kind == "dense":
        dense = _setup(engine, _dense_sweep_case(key, d))
    else:
        dense = _setup(engine, sc.mixed_pattern_coeffs(key, d, True), sparse=True)
    N = dense[0].shape[0]
    nA = np.linalg.norm(pr.companion(dense)[0])
    unit = 16 * d * N * EPS
    Q = pc.random_block(N, r, 47)
    dQ = engine.upload(Q)
    Ahat = engine.poly_project_reduced(dQ, r)
    assert len(Ahat) == d + 1
    for k in range(d + 1):
        err = np.linalg.norm(Ahat[k] - Q.conj().T @ (dense[k] @ Q))
        print("Ahat_%d: error %.2e bound %.2e" % (k, err, unit * nA * np.linalg.norm(Q) ** 2))
        assert Ahat[k].shape == (r, r) and err <= unit * nA * np.linalg.norm(Q) ** 2
    ncand = d * r
    rng = np.random.default_rng(53)
    Y = np.asfortranarray(rng.standard_normal((r, ncand)) + 1j * rng.standard_normal((r, ncand)))
    theta = 0.2 + 0.1j + 0.7 * (rng.uniform(-1, 1, ncand) + 1j * rng.uniform(-1, 1, ncand))
    theta[ncand - 2] = np.inf
    Y[:, ncand - 1] = 0.0                                     # a candidate without a vector
    Xr = Q @ Y
    nrm = np.linalg.norm(Xr, axis=0)
    live = nrm > 0
    Xr[:, live] /= nrm[live]
    be_ref = ppr.candidate_errors(dense, theta, Xr)
    dX, be = engine.poly_ritz_eval(dQ, r, Y, theta)
    Xg = engine.download(dX, ncand)
    xerr = np.abs(Xg - Xr).max()
    xbound = unit * np.linalg.norm(Q) * np.linalg.norm(Y) / nrm[live].min()
    fin = np.isfinite(be_ref) & live
    print("r %d ncand %d: X error %.2e (bound %.2e), backward error difference %.2e (bound %.2e)" % (
        r, ncand, xerr, xbound, np.abs(be[fin] - be_ref[fin]).max(), unit))
    assert Xg.shape == (N, ncand) and xerr <= xbound
    assert np.abs(be[fin] - be_ref[fin]).max() <= unit
    assert np.isposinf(be[ncand - 2]) and np.isposinf(be[ncand - 1]) and fin.sum() == ncand - 2
    # without theta: the vectors alone, the same ones
    dX2, none = engine.poly_ritz_eval(dQ, r, Y)
    assert none is None and np.array_equal(engine.download(dX2, ncand), Xg)


def test_poly_orthonormalize(engine, restore):
    """the N x m orthonormalisation of a polynomial handle, by both methods, on a block of rank 9 in 12 columns of very
    different lengths, and over the 64-column panel"""
    N = 193
    _setup(engine, _dense_sweep_case(N, 2))
    B = pc.random_block(N, 9, 59)
    rng = np.random.default_rng(61)
    X = np.asfortranarray((B @ (rng.standard_normal((9, 12)) + 1j * rng.standard_normal((9, 12)))) * 10.0 ** rng.uniform(-6, 6, 12)[None, :])
    for method in ("mgs", "cholqr_rr"):
        engine.set_ortho_method(method)
        dQ = engine.upload(X)
        rank = engine.poly_orthonormalize(dQ, 12, ppr.RANK_TOL)
        Q = engine.download(dQ, 12)[:, :rank]
        defect = np.linalg.norm(Q.conj().T @ Q - np.eye(rank))
        span = np.linalg.norm(B - Q @ (Q.conj().T @ B)) / np.linalg.norm(B)
        print("%s: rank %d, ||Q^H Q - I|| %.2e, span defect %.2e, last_ortho %s" % (method, rank, defect, span, engine.last_ortho()))
        assert rank == 9 and engine.last_ortho()["rank"] == 9
        assert defect <= 64 * N * EPS and span <= 1e3 * N * EPS
    engine.set_ortho_method("mgs")
    W = pc.random_block(N, 72, 67)
    dQ = engine.upload(W)
    assert engine.poly_orthonormalize(dQ, 72, ppr.RANK_TOL) == 72
    Q = engine.download(dQ, 72)
    assert np.linalg.norm(Q.conj().T @ Q - np.eye(72)) <= 64 * N * EPS


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def _fpm(fpm3, ne=pc.NE):
    fpm = fk.feastinit()
    fpm[8], fpm[3] = ne, fpm3
    return fpm


def _check_result(res, ref, dense, lam_in, ne):
    """a device run against the restatement's run and numpy on its vectors"""
    poly = res.stats["polynomial"]
    N, d = dense[0].shape[0], len(dense) - 1
    lam_err = pr.match_error(res.lambda_, lam_in) if res.M == len(lam_in) else np.inf
    be_np = pr.backward_error(dense, res.lambda_, res.q)
    print("loop %d (restatement %d) history %s (restatement %s) rank %s set aside %s eigenvalue error %.2e factorizations %d" % (
        res.loop, ref["loop"], ["%.1e" % e for e in poly["eps_history"]], ["%.1e" % e for e in ref["eps_history"]], poly["rank"],
        poly["set_aside"], lam_err, res.stats["factorizations"]))
    assert res.info == ref["info"] == 0 and res.M == ref["M"] == len(lam_in)
    assert res.loop == ref["loop"]
    assert lam_err <= 1e-8
    assert res.q.shape == (N, res.M) and np.abs(np.linalg.norm(res.q, axis=0) - 1.0).max() <= 16 * N * EPS
    # res is the backward error of the returned pairs: numpy agrees to 3 digits (above the rounding of the evaluation itself)
    assert np.all(np.abs(be_np - res.res) <= 1e-3 * res.res + 16 * d * N * EPS)
    assert np.array_equal(poly["backward_error"], res.res) and res.epsout == res.res.max() == poly["eps_history"][-1]
    assert poly["method"] == "projected" and poly["degree"] == d
    assert len(poly["eps_history"]) == len(poly["rank"]) == len(poly["candidates"]) == len(poly["set_aside"]) == res.loop + 1
    assert poly["candidates"] == [d * r for r in poly["rank"]] and poly["rank"] == ref["rank"]
    assert res.stats["factorizations"] == ne


@pytest.mark.parametrize("seed", ppr.SEEDS)
@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_driver_dense(engine, restore, params, seed):
    N, d, k, _, monic = params
    key = (N, d, k, monic)
    fpm3, loop = ppr.DENSE_PINS[key]
    case = pc.make_case(*key)
    ref = ppr.dense_run(key, k + 2, seed, fpm3)
    assert ref["loop"] == loop
    Q0 = fo.seeded_subspace(N, k + 2, seed)
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=k + 2, fpm=_fpm(fpm3), engine=engine, Q0=Q0, method="projected")
    _check_result(res, ref, case["coeffs"], case["lam_in"], pc.NE)
    assert res.stats["polynomial"]["columns"] == k + 2 and "plan" not in res.stats["polynomial"]
    if seed == 1:
        rr = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=k + 2, fpm=_fpm(fpm3), engine=engine, Q0=Q0,
                                 method="projected", ortho="cholqr_rr")
        print("cholqr_rr: loop %d M %d, ortho %s" % (rr.loop, rr.M, [o["method"] for o in rr.stats["ortho"]]))
        assert rr.info == 0 and rr.M == res.M and rr.loop == res.loop
        assert len(rr.stats["ortho"]) == rr.loop + 1 and pr.match_error(rr.lambda_, case["lam_in"]) <= 1e-8


@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES, ids=sc.DRIVER_IDS)
def test_driver_sparse(engine, restore, name, scaled):
    columns, seed, loop = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    ref = ppr.damped_run(name, scaled, columns, seed)
    assert ref["loop"] == loop
    Q0 = fo.seeded_subspace(case["N"], columns, seed)
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=columns, fpm=_fpm(sc.FPM3, sc.NE), engine=engine, Q0=Q0,
                              solver="sparse_direct", method="projected")
    _check_result(res, ref, sc.dense(case["coeffs"]), case["lam_in"], sc.NE)
    poly = res.stats["polynomial"]
    assert poly["plan"] == "multifrontal" and poly["fell_back"] is False and "solver_substitution" not in res.stats
    assert poly["plan_nnz"] == len(polynomial_union_csr(case["coeffs"])[1]) and poly["plan_factor_bytes"] > 0 and poly["plan_flops"] > 0
    assert poly["columns"] == columns


def test_driver_fallback_to_the_dense_expansion(engine, restore, monkeypatch):
    """the saddle-point quadratic: the multifrontal LU rejects a pivot, the projected run repeats on the dense expansion"""
    monkeypatch.setenv("FH_MF_LEAF", "8")
    case = sc.saddle_quadratic()
    k = len(case["lam_in"])
    res = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], M0=k + 2, fpm=_fpm(sc.FPM3, sc.NE), engine=engine,
                              solver="sparse_direct", method="projected")
    poly = res.stats["polynomial"]
    lam_err = pr.match_error(res.lambda_, case["lam_in"]) if res.M == k else np.inf
    print("M %d loop %d epsout %.2e eigenvalue error %.2e; %s" % (res.M, res.loop, res.epsout, lam_err, res.stats.get("solver_substitution")))
    assert poly["fell_back"] is True and poly["plan"] == "dense" and poly["method"] == "projected"
    assert res.stats["solver_substitution"]["requested"] == "sparse_direct" and "pivot" in res.stats["solver_substitution"]["reason"]
    assert res.info == 0 and res.M == k and res.epsout <= 1e-10 and lam_err <= 1e-8


def test_linearised_is_unchanged_and_single_precision(engine, restore):
    N, d, k, M0, monic = pc.DRIVER_CASES[0]
    case = pc.make_case(N, d, k, monic)
    args = (case["coeffs"], case["center"], case["radius"])
    a = fk.feast_polynomial(*args, M0=M0, fpm=_fpm(pc.FPM3), engine=engine)
    b = fk.feast_polynomial(*args, M0=M0, fpm=_fpm(pc.FPM3), engine=engine, method="linearised")
    assert a.info == b.info == 0 and a.loop == b.loop and a.M == b.M == k
    assert np.array_equal(a.lambda_, b.lambda_) and np.array_equal(a.q, b.q) and np.array_equal(a.res, b.res)
    assert a.stats["polynomial"]["method"] == "linearised" and a.stats["polynomial"]["columns"] == M0 * d
    # complex64 input: promoted, solved at the single-precision floor, demoted
    single = [c.astype(np.complex64) for c in case["coeffs"]]
    s = fk.feast_polynomial(single, case["center"], case["radius"], M0=k + 2, fpm=_fpm(pc.FPM3), engine=engine, method="projected")
    assert s.info == 0 and s.M == k and s.lambda_.dtype == np.complex64 and s.q.dtype == np.complex64
    assert s.epsout <= np.sqrt(np.finfo(np.float32).eps)


def test_loop_limit_returns_the_last_iterates(engine, restore):
    N, d, k, _, monic = pc.DRIVER_CASES[0]
    case = pc.make_case(N, d, k, monic)
    fpm = _fpm(pc.FPM3)
    fpm[4] = 1
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=k + 2, fpm=fpm, engine=engine, Q0=fo.seeded_subspace(N, k + 2, 1),
                              method="projected")
    assert res.info == int(fk.FeastError.Feast_ERROR_NO_CONVERGENCE) and res.loop == 1 and res.M == k
    assert 1e-10 < res.epsout < 1e-7 and pr.match_error(res.lambda_, case["lam_in"]) <= 1e-6


def test_refusals(engine, restore):
    N, m = 70, 5
    X = pc.random_block(N, m, 71)
    lam = _lambdas(m)
    # a pencil handle takes none of the polynomial calls
    engine.set_problem(np.diag(np.arange(1.0, N + 1)))
    engine.set_solver("direct")
    Zne, Wne = fo.feast_gcontour(pc.CENTER, pc.RADIUS, 8)
    engine.set_contour(Zne, Wne, 1.0)
    dX = engine.upload(X)
    calls = [lambda: engine.poly_eval_cols(dX, lam, m), lambda: engine.poly_resinv_apply(dX, m), lambda: engine.poly_resinv_apply(dX, m, lam),
             lambda: engine.poly_ritz_eval(dX, m, np.eye(m), lam), lambda: engine.poly_orthonormalize(dX, m, 1e-8)]
    calls.append(lambda: engine.poly_project_reduced(dX, m))
    for call in calls:
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "polynomial handle" in str(err.value)
    # a polynomial handle: widths out of range, and the pencil's orthonormalisation stays refused
    _setup(engine, pc.random_coeffs(N, 2, True), (Zne, Wne))
    dW = engine.upload(pc.random_block(N, N, 73))
    for call in (lambda: engine.poly_project_reduced(dW, N + 1), lambda: engine.poly_orthonormalize(dW, N + 1, 1e-8),
                 lambda: engine.poly_resinv_apply(dX, 0)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == 2
    with pytest.raises(FeastHipError) as err:
        engine.orthonormalize(dX, m, 1e-8)
    assert err.value.code == FPM_ERROR
    engine.set_real_projection(True)
    with pytest.raises(FeastHipError) as err:
        engine.poly_resinv_apply(dX, m)
    assert err.value.code == FPM_ERROR and "real projection" in str(err.value)
    engine.set_real_projection(False)
    _, status, _ = engine.poly_resinv_apply(dX, m)
    assert not status.any()
