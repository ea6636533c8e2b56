"""feast_polynomial on the device: the feasthip_poly_* primitives against numpy on the explicit companion pencil, the factor
cache, the driver against the constructed spectra and the restatement of tests/polynomial_reference.py, parity with the
oracle's feast_general on the companion, and the refusals of the ABI."""
import numpy as np
import pytest

import feast_oracle as fo
import feastkit_jl_amd as fk
import polynomial_cases as pc
import polynomial_reference as pr
from feastkit_jl_amd.types import FeastHipError

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FPM_ERROR = 9


def _fpm(fpm4=None):
    fpm = fk.feastinit()
    fpm[8], fpm[3] = pc.NE, pc.FPM3
    if fpm4 is not None:
        fpm[4] = fpm4
    return fpm


def _contour(ne=pc.NE):
    return fo.feast_gcontour(pc.CENTER, pc.RADIUS, ne)


def _setup(engine, coeffs, ne=pc.NE):
    engine.set_adjoint(False)
    engine.set_polynomial(coeffs)
    engine.set_solver("direct", cache_factors=True, factor_precision=64)
    engine.set_real_projection(False)
    Zne, Wne = _contour(ne)
    engine.set_contour(Zne, Wne, 1.0)
    return Zne, Wne


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")


@pytest.mark.parametrize("m", [5, 64])
@pytest.mark.parametrize("N,d,cplx", pc.SOLVE_SHAPES)
def test_poly_solve(engine, restore, N, d, cplx, m):
    coeffs = pc.random_coeffs(N, d, cplx)
    Zne, _ = _setup(engine, coeffs)
    z = Zne[3]
    R = pc.random_block(N, m, 11)
    dY, rc = engine.poly_solve(z, engine.upload(R), m)
    Y = engine.download(dY, m)
    P = pr.poly_at(coeffs, z)
    berr = np.linalg.norm(P @ Y - R) / (np.linalg.norm(P) * np.linalg.norm(Y) + np.linalg.norm(R))
    print("N %d d %d m %d backward error %.2e bound %.2e" % (N, d, m, berr, 64 * N * EPS))
    assert rc == 0
    assert berr <= 64 * N * EPS
    if d == 1:
        engine.set_problem(-coeffs[0], coeffs[1])
        engine.set_solver("direct", cache_factors=True, factor_precision=64)
        dY2, rc2 = engine.shifted_solve(z, engine.upload(R), m)
        Y2 = engine.download(dY2, m)
        cond = np.linalg.cond(P)
        diff = np.linalg.norm(Y - Y2) / np.linalg.norm(Y2)
        print("against shifted_solve on (-A_0, A_1): %.2e, cond %.2e" % (diff, cond))
        assert rc2 == 0 and diff <= 64 * N * EPS * cond


def _sweep_case(N, d):
    k = {70: 6, 45: 7, 193: 9}[N]
    return pc.make_case(N, d, k, False)


@pytest.mark.parametrize("ne", [8, 16])
@pytest.mark.parametrize("N,d,m", pc.SWEEP_SHAPES)
def test_poly_contour_apply(engine, restore, N, d, m, ne):
    coeffs = _sweep_case(N, d)["coeffs"]
    Zne, Wne = _setup(engine, coeffs, ne)
    Q = pc.random_block(d * N, m, 13)
    ref, conds = pr.contour_sum(coeffs, Zne, Wne, Q)
    dP, status, st = engine.poly_contour_apply(engine.upload(Q), m)
    P = engine.download(dP, m)
    err = np.linalg.norm(P - ref) / np.linalg.norm(ref)
    print("N %d d %d m %d ne %d: cond max %.2e, relative error %.2e, bound %.2e" % (N, d, m, ne, conds.max(), err, 1e3 * EPS * conds.max()))
    assert not status[:ne].any() and st["factorizations"] == ne
    assert P.shape == (d * N, m)
    assert err <= 1e3 * EPS * conds.max()


@pytest.mark.parametrize("N,d,m", pc.SWEEP_SHAPES)
def test_products_projection_residual(engine, restore, N, d, m):
    coeffs = _sweep_case(N, d)["coeffs"]
    _setup(engine, coeffs)
    A, B = pr.companion(coeffs)
    nA, nB = np.linalg.norm(A), np.linalg.norm(B)
    unit = 16 * d * N * EPS
    X = pc.random_block(d * N, m, 17)
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
    lam = pc.CENTER + 0.7 * (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m))
    M = m - 3
    Xr = X @ V
    nrm = np.linalg.norm(Xr, axis=0)
    Xr[:, :M] /= nrm[:M]
    bwd_ref = pr.backward_error(coeffs, lam[:M], Xr[:N, :M])
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
    N, d, m = 70, 2, 12
    coeffs = _sweep_case(N, d)["coeffs"]
    _setup(engine, coeffs)
    dQ = engine.upload(pc.random_block(d * N, m, 23))
    dP1, _, st1 = engine.poly_contour_apply(dQ, m)
    dP2, _, st2 = engine.poly_contour_apply(dQ, m)
    assert st1["factorizations"] == pc.NE and st2["factorizations"] == 0
    assert np.array_equal(engine.download(dP1, m), engine.download(dP2, m))
    engine.free_factors()
    _, _, st3 = engine.poly_contour_apply(dQ, m)
    assert st3["factorizations"] == pc.NE


@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_driver(engine, restore, params):
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    ref = pr.driver_run(params)
    Q0 = fo.seeded_subspace(d * N, M0 * d, 20260515)
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=M0, fpm=_fpm(), engine=engine, Q0=Q0)
    poly = res.stats["polynomial"]
    lam_err = pr.match_error(res.lambda_, case["lam_in"])
    bwd_np = pr.backward_error(case["coeffs"], res.lambda_, res.q)
    print("loop %d (restatement %d) epsout %.2e history %s eigenvalue error %.2e backward error %.2e (numpy on q: %.2e) factorizations %d" % (
        res.loop, ref["loop"], res.epsout, ["%.1e" % e for e in poly["eps_history"]], lam_err, poly["backward_error"].max(), bwd_np.max(),
        res.stats["factorizations"]))
    assert res.info == 0 and res.M == k
    assert abs(res.loop - ref["loop"]) <= 1
    assert res.epsout <= 1e-10
    assert lam_err <= 1e-9
    assert poly["backward_error"].max() <= 1e-11
    assert res.q.shape == (N, k)
    assert np.abs(bwd_np - poly["backward_error"]).max() <= 16 * d * N * EPS
    assert poly["degree"] == d and poly["columns"] == M0 * d and poly["residual"] == "pencil"
    assert len(poly["eps_history"]) == res.loop + 1
    assert res.stats["factorizations"] == pc.NE


@pytest.mark.parametrize("params", [p for p in pc.DRIVER_CASES if p[4]], ids=[i for p, i in zip(pc.DRIVER_CASES, pc.DRIVER_IDS) if p[4]])
def test_reference_parity_monic(engine, restore, params):
    N, d, k, M0, monic = params
    case = pc.make_case(N, d, k, monic)
    A, B = pr.companion(case["coeffs"])
    Q0 = fo.seeded_subspace(d * N, M0 * d, 20260515)
    ref = fo.feast_general(A, B, case["center"], case["radius"], M0 * d, ne=pc.NE, fpm3=pc.FPM3, Q0=Q0)
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=M0, fpm=_fpm(), engine=engine, Q0=Q0, residual="reference")
    print("loop %d (oracle %d) epsout %.2e (oracle %.2e)" % (res.loop, ref.loop, res.epsout, ref.epsout))
    assert res.info == ref.info == 0 and res.M == ref.M
    assert abs(res.loop - ref.loop) <= 1
    assert pr.match_error(res.lambda_, ref.lam) <= 1e-9


def test_reference_parity_nonmonic_quadratic(engine, restore):
    """The reference's residual omits B_lin and never falls for A_d != I: both sides run into the loop limit."""
    N, d, k, M0, monic = pc.DRIVER_CASES[1]
    case = pc.make_case(N, d, k, monic)
    A, B = pr.companion(case["coeffs"])
    Q0 = fo.seeded_subspace(d * N, M0 * d, 20260515)
    ref = fo.feast_general(A, B, case["center"], case["radius"], M0 * d, ne=pc.NE, fpm3=pc.FPM3, fpm4=3, Q0=Q0)
    res = fk.feast_polynomial(case["coeffs"], case["center"], case["radius"], M0=M0, fpm=_fpm(3), engine=engine, Q0=Q0, residual="reference")
    print("loop %d / %d, epsout %.2e / %.2e, M %d / %d" % (res.loop, ref.loop, res.epsout, ref.epsout, res.M, ref.M))
    assert res.loop == ref.loop == 3
    assert res.info == ref.info == 0 and res.M == ref.M
    assert pr.match_error(res.lambda_, ref.lam) <= 1e-8


def test_abi_refusals(engine, restore):
    N, d, m = 45, 3, 5
    coeffs = _sweep_case(N, d)["coeffs"]
    _setup(engine, coeffs)
    dN = engine.upload(pc.random_block(N, m, 29))
    V, lam = np.eye(m, dtype=complex), np.zeros(m, dtype=complex)
    pencil_calls = [lambda: engine.contour_apply(dN, m), lambda: engine.contour_apply_resident(dN, m), lambda: engine.project(dN, m),
                    lambda: engine.project_pair(dN, dN, m), lambda: engine.matmul(0, dN, m), lambda: engine.shifted_solve(0.5j, dN, m),
                    lambda: engine.ritz_residual(dN, m, V, lam, m), lambda: engine.orthonormalize(dN, m, 1e-8),
                    lambda: engine.rayleigh_ritz(dN, m, -1.0, 1.0), lambda: engine.estimate_count(m, 1), lambda: engine.random_block(m, 1),
                    lambda: engine.rr_reduce_resident(m, 1e-8), lambda: engine.import_resident(dN, m), lambda: engine.export_resident(m)]
    for call in pencil_calls:
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "feasthip_poly_" in str(err.value)
    for call in (lambda: engine.set_adjoint(True), lambda: engine.set_node_range(0, 4), lambda: engine.set_node_list([0, 2]),
                 lambda: engine.set_solver("direct", factor_precision=32), lambda: engine.set_solver("bicgstab")):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "polynomial" in str(err.value)
    # none of the refused settings took hold: the handle still sweeps
    dQ = engine.upload(pc.random_block(d * N, m, 31))
    _, status, _ = engine.poly_contour_apply(dQ, m)
    assert not status.any()
    # settings made BEFORE the polynomial was installed are caught by the poly_ calls themselves
    T = np.diag(np.arange(1.0, 9.0))
    engine.set_problem(T)
    engine.set_solver("direct", factor_precision=32)
    engine.set_polynomial(coeffs)
    with pytest.raises(FeastHipError) as err:
        engine.poly_contour_apply(dQ, m)
    assert err.value.code == FPM_ERROR and "factor_precision" in str(err.value)
    engine.set_solver("direct", factor_precision=64)
    # a poly_ call on a dense handle
    engine.set_problem(T)
    engine.poly_degree = 1
    for call in (lambda: engine.poly_contour_apply(engine.upload(np.eye(8, 2)), 2), lambda: engine.poly_matmul(0, engine.upload(np.eye(8, 2)), 2),
                 lambda: engine.poly_project(engine.upload(np.eye(8, 2)), 2), lambda: engine.poly_solve(0.5j, engine.upload(np.eye(8, 2)), 2),
                 lambda: engine.poly_ritz_residual(engine.upload(np.eye(8, 2)), 2, np.eye(2), np.zeros(2), 2)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "feasthip_set_polynomial" in str(err.value)
    # and the engine is an ordinary one again
    res = fk.feast_general(T, None, 2.5, 1.0, M0=4, engine=engine)
    assert res.info == 0 and res.M == 2 and np.abs(np.sort(res.lambda_.real) - [2.0, 3.0]).max() <= 1e-10
