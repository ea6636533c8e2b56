"""feast_nonlinear on the device: the feasthip_nep_* calls on dense and sparse term handles (k_form_terms / k_mf_assemble_terms
behind the solves, k_spmm_terms / the dense products on column-scaled panels, k_poly_resinv_acc on the cached factors, the
candidate evaluation) against numpy, the refusals, and the driver on the closed-form cases of tests/nonlinear_cases.py held to
the numpy restatement of tests/nonlinear_reference.py.  The bounds of the primitives are those tests/test_gpu_polynomial_projected.py
uses for the same primitive on a polynomial handle -- 16 nterms N eps ||A|| ||X|| for products, 1e3 eps cond_2 for solves and
contour sums: the arithmetic differs only in how the scalar is formed."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import feast_oracle as fo
import feastkit_jl_amd as fk
import nonlinear_cases as nc
import nonlinear_reference as nr
import polynomial_cases as pc
import polynomial_projected_reference as ppr
import polynomial_sparse_cases as sc
from feastkit_jl_amd.ingest import polynomial_union_csr
from feastkit_jl_amd.types import FeastHipError

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
FPM_ERROR = 9
NE = 8                      # contour of the primitive tests
GRID = (6, 5, 4)
# (kind, key, nterms, complex matrices): dense N = 70 and 45, CSR on the 6 x 5 x 4 grid, nterms 2, 3 and 9, real and complex
SHAPES = [("dense", 70, 2, True), ("dense", 45, 3, False), ("dense", 45, 9, True), ("dense", 70, 9, False),
          ("sparse", GRID, 2, False), ("sparse", GRID, 3, True), ("sparse", GRID, 9, True), ("sparse", GRID, 9, False)]
WIDTHS = [1, 63, 64, 65, 130]          # the panel edges and a block of three panels


@pytest.fixture
def restore(engine):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_solver("direct")
    engine.set_ortho_method("mgs")


@functools.lru_cache(maxsize=None)
def _problem(kind, key, nterms, cplx):
    """-> (terms as the engine takes them, dense matrices, functions, (Zne, Wne), centre, radius, F_node); shared, not to be modified"""
    if kind == "dense":
        terms = nc.random_terms(key, nterms, cplx)
        center, radius = pc.CENTER, pc.RADIUS
    else:
        # A_0 + lambda A_1 = L + 4 I - lambda I + small couplings keeps its eigenvalues inside sweep_circle, as in the polynomial
        # tests (a contour sum around nothing is a cancelling sum, and a bound relative to its norm would mean nothing); the other
        # terms, small against A_0, get the functions of nonlinear_cases.random_terms
        mats = sc.mixed_pattern_coeffs(key, nterms - 1, cplx)
        other = [f for _, f in nc.random_terms(4, 9, False)]
        terms = list(zip(mats, ([other[0], 1] + other[2:])[:nterms]))
        center, radius = sc.sweep_circle(key)
    dense, funcs = nr.split(terms)
    contour = fo.feast_gcontour(center, radius, NE)
    return terms, dense, funcs, contour, center, radius, nr.table(funcs, contour[0])


def _install(engine, terms, contour=None, F_node=None):
    engine.set_adjoint(False)
    mats = [A for A, _ in terms]
    if sp.issparse(mats[0]):
        engine.set_terms_csr(*polynomial_union_csr(mats))
    else:
        engine.set_terms(mats)
    engine.set_solver("direct", cache_factors=True, factor_precision=64)
    engine.set_real_projection(False)
    if contour is not None:
        engine.set_contour(contour[0], contour[1], 1.0)
        engine.nep_set_node_values(F_node)


def _setup(engine, kind, key, nterms, cplx):
    terms, dense, funcs, contour, center, radius, F_node = _problem(kind, key, nterms, cplx)
    _install(engine, terms, contour, F_node)
    return dense, funcs, contour, center, radius, F_node


def _points(center, radius, m):
    """one value per column inside the circle, none on a node"""
    j = np.arange(m)
    return center + radius * (0.15 + 0.6 * j / m) * np.exp(2j * np.pi * (j * 0.381966 + 0.05))


# ---- sum_k F[j, k] A_k x_j -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("kind,key,nterms,cplx", SHAPES)
def test_nep_eval_cols(engine, restore, kind, key, nterms, cplx, m):
    dense, funcs, _, center, radius, _ = _setup(engine, kind, key, nterms, cplx)
    N = dense[0].shape[0]
    F = nr.table(funcs, _points(center, radius, m))
    X = pc.random_block(N, m, 41)
    dX = engine.upload(X)
    R = engine.download(engine.nep_eval_cols(dX, F, m), m)
    ref = nr.eval_cols(dense, F, X)
    bound = 16 * nterms * N * EPS * sum(np.linalg.norm(Ak) * np.linalg.norm(X * np.abs(F[None, :, k])) for k, Ak in enumerate(dense))
    err = np.linalg.norm(R - ref)
    print("%s nterms %d m %d: error %.2e bound %.2e" % (key, nterms, m, err, bound))
    assert R.shape == (N, m) and err <= bound
    assert np.array_equal(R, engine.download(engine.nep_eval_cols(dX, F, m), m))


# ---- T(z_e)^-1 R and the contour step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("kind,key,nterms,cplx", SHAPES)
def test_nep_solve(engine, restore, kind, key, nterms, cplx, m):
    dense, _, _, _, _, F_node = _setup(engine, kind, key, nterms, cplx)
    N = dense[0].shape[0]
    Rhs = pc.random_block(N, m, 43)
    dR = engine.upload(Rhs)
    for node, nfact in ((NE - 1, 1), (2, 1), (NE - 1, 0)):          # the third solve finds the first one's factor
        T = nr.t_at(dense, F_node[node])
        dY, code = engine.nep_solve(node, dR, m)
        Y = engine.download(dY, m)
        ref = np.linalg.solve(T, Rhs)
        cond = np.linalg.cond(T)
        err = np.linalg.norm(Y - ref) / np.linalg.norm(ref)
        print("%s nterms %d m %d node %d: cond %.2e error %.2e bound %.2e" % (key, nterms, m, node, cond, err, 1e3 * EPS * cond))
        assert code == 0 and err <= 1e3 * EPS * cond and engine.last_stats["factorizations"] == nfact


@functools.lru_cache(maxsize=None)
def _sweep_reference(kind, key, nterms, cplx, m):
    _, dense, funcs, (Zne, Wne), center, radius, F_node = _problem(kind, key, nterms, cplx)
    X = pc.random_block(dense[0].shape[0], m, 47)
    sigma = _points(center, radius, m)
    F_sigma = nr.table(funcs, sigma)
    cond = max(np.linalg.cond(nr.t_at(dense, F_node[e])) for e in range(NE))
    return X, sigma, F_sigma, nr.sweep(dense, F_node, Zne, Wne, X), nr.sweep(dense, F_node, Zne, Wne, X, sigma, F_sigma), cond


@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("kind,key,nterms,cplx", SHAPES)
def test_nep_resinv_apply(engine, restore, kind, key, nterms, cplx, m):
    _, _, contour, _, _, _ = _setup(engine, kind, key, nterms, cplx)
    X, sigma, F_sigma, plain, shifted, cond = _sweep_reference(kind, key, nterms, cplx, m)
    engine.free_factors()
    dX = engine.upload(X)
    dQ, status, st1 = engine.nep_resinv_apply(dX, m)
    Q = engine.download(dQ, m)
    err = np.linalg.norm(Q - plain) / np.linalg.norm(plain)
    print("%s nterms %d m %d: cond max %.2e, plain sweep error %.2e, bound %.2e" % (key, nterms, m, cond, err, 1e3 * EPS * cond))
    assert not status[:NE].any() and st1["factorizations"] == NE
    assert Q.shape == X.shape and err <= 1e3 * EPS * cond
    dS, status, st2 = engine.nep_resinv_apply(dX, m, sigma, F_sigma)
    S = engine.download(dS, m)
    err = np.linalg.norm(S - shifted) / np.linalg.norm(shifted)
    print("shifted sweep error %.2e" % err)
    assert not status[:NE].any() and st2["factorizations"] == 0          # the cached factors
    assert err <= 1e3 * EPS * cond
    assert np.array_equal(S, engine.download(engine.nep_resinv_apply(dX, m, sigma, F_sigma)[0], m))
    # a shift on a node is refused on the host, nothing is divided by zero on the device
    bad = sigma.copy()
    bad[m // 2] = contour[0][NE // 2]
    with pytest.raises(FeastHipError) as err:
        engine.nep_resinv_apply(dX, m, bad, F_sigma)
    assert err.value.code == FPM_ERROR and "coincides with contour node %d" % (NE // 2) in str(err.value)


# ---- the candidates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncand", WIDTHS)
@pytest.mark.parametrize("r", [7, 72])
@pytest.mark.parametrize("kind,key,nterms,cplx", SHAPES)
def test_nep_ritz_eval_and_projection(engine, restore, kind, key, nterms, cplx, r, ncand):
    dense, funcs, _, center, radius, _ = _setup(engine, kind, key, nterms, cplx)
    N = dense[0].shape[0]
    r = min(r, N)
    unit = 16 * nterms * N * EPS
    Q = pc.random_block(N, r, 53)
    dQ = engine.upload(Q)
    Ahat = engine.poly_project_reduced(dQ, r)          # takes a term handle as it is
    nA = np.sqrt(sum(np.linalg.norm(A) ** 2 for A in dense))
    assert len(Ahat) == nterms
    for k in range(nterms):
        assert np.linalg.norm(Ahat[k] - Q.conj().T @ (dense[k] @ Q)) <= unit * nA * np.linalg.norm(Q) ** 2
    # ncand: the panel edges and three panels of candidates; more candidates than columns is what two Beyn moments give
    rng = np.random.default_rng(59)
    Y = np.asfortranarray(rng.standard_normal((r, ncand)) + 1j * rng.standard_normal((r, ncand)))
    F = nr.table(funcs, _points(center, radius, ncand))
    special = 2 if ncand > 2 else 0
    if special:
        F[ncand - 2, nterms - 1] = np.inf              # a row that is not finite
        Y[:, ncand - 1] = 0.0                          # a candidate without a vector
    Xr = Q @ Y
    nrm = np.linalg.norm(Xr, axis=0)
    live = nrm > 0
    Xr[:, live] /= nrm[live]
    be_ref = nr.candidate_errors(dense, F, Xr)
    dX, be = engine.nep_ritz_eval(dQ, r, Y, F)
    Xg = engine.download(dX, ncand)
    xerr = np.abs(Xg - Xr).max()
    xbound = unit * np.linalg.norm(Q) * np.linalg.norm(Y) / nrm[live].min()
    fin = np.isfinite(be_ref) & live
    print("%s nterms %d r %d ncand %d: X error %.2e (bound %.2e), backward error difference %.2e (bound %.2e)" % (
        key, nterms, r, ncand, xerr, xbound, np.abs(be[fin] - be_ref[fin]).max(), unit))
    assert Xg.shape == (N, ncand) and xerr <= xbound
    assert np.abs(be[fin] - be_ref[fin]).max() <= unit
    assert fin.sum() == ncand - special and (not special or (np.isposinf(be[ncand - 2]) and np.isposinf(be[ncand - 1])))
    dX2, none = engine.nep_ritz_eval(dQ, r, Y)
    assert none is None and np.array_equal(engine.download(dX2, ncand), Xg)
    # the pencil's orthonormalisation of a term handle's block
    dW = engine.upload(Q)
    assert engine.poly_orthonormalize(dW, r, ppr.RANK_TOL) == r
    W = engine.download(dW, r)
    assert np.linalg.norm(W.conj().T @ W - np.eye(r)) <= 64 * N * EPS


# ---- a polynomial posed as terms agrees with the polynomial primitives -----------------------------------------------------------
@pytest.mark.parametrize("kind,key,d", [("dense", 70, 2), ("dense", 45, 8), ("sparse", GRID, 3)])
def test_polynomial_posed_as_terms(engine, restore, kind, key, d):
    m = 65
    if kind == "dense":
        coeffs = pc.make_case(key, d, 6, False)["coeffs"] if d == 2 else pc.random_coeffs(key, d, True)
        dense, center, radius = list(coeffs), pc.CENTER, pc.RADIUS
    else:
        coeffs = sc.mixed_pattern_coeffs(key, d, True)
        dense = sc.dense(coeffs)
        center, radius = sc.sweep_circle(key)
    N = dense[0].shape[0]
    m = min(m, N)          # (the candidate evaluation takes at most N columns)
    contour = fo.feast_gcontour(center, radius, NE)
    funcs = [nr.as_function(k) for k in range(d + 1)]
    X = pc.random_block(N, m, 61)
    sigma = _points(center, radius, m)
    dX = engine.upload(X)
    engine.set_adjoint(False)
    if kind == "dense":
        engine.set_polynomial(coeffs)
    else:
        engine.set_polynomial_csr(*polynomial_union_csr(coeffs))
    engine.set_solver("direct", cache_factors=True, factor_precision=64)
    engine.set_real_projection(False)
    engine.set_contour(contour[0], contour[1], 1.0)
    Rp = engine.download(engine.poly_eval_cols(dX, sigma, m), m)
    Qp = engine.download(engine.poly_resinv_apply(dX, m)[0], m)
    Sp = engine.download(engine.poly_resinv_apply(dX, m, sigma)[0], m)
    _, bep = engine.poly_ritz_eval(dX, m, np.eye(m), sigma)
    engine.free_factors()
    _install(engine, list(zip(coeffs, funcs)), contour, nr.table(funcs, contour[0]))
    Fs = nr.table(funcs, sigma)
    Rt = engine.download(engine.nep_eval_cols(dX, Fs, m), m)
    Qt = engine.download(engine.nep_resinv_apply(dX, m)[0], m)
    St = engine.download(engine.nep_resinv_apply(dX, m, sigma, Fs)[0], m)
    _, bet = engine.nep_ritz_eval(dX, m, np.eye(m), Fs)
    cond = max(np.linalg.cond(sum(z ** k * A for k, A in enumerate(dense))) for z in contour[0])
    ebound = 16 * d * N * EPS * sum(np.linalg.norm(Ak) * np.linalg.norm(X * np.abs(sigma)[None, :] ** k) for k, Ak in enumerate(dense))
    errs = (np.linalg.norm(Rt - Rp), np.linalg.norm(Qt - Qp) / np.linalg.norm(Qp), np.linalg.norm(St - Sp) / np.linalg.norm(Sp), np.abs(bet - bep).max())
    print("%s d %d: eval %.2e (bound %.2e), plain %.2e shifted %.2e (bound %.2e), backward error %.2e" % ((key, d, errs[0], ebound) + errs[1:3] + (1e3 * EPS * cond, errs[3])))
    assert errs[0] <= ebound and errs[1] <= 1e3 * EPS * cond and errs[2] <= 1e3 * EPS * cond and errs[3] <= 16 * d * N * EPS


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(engine, restore):
    N, m, nterms = 70, 5, 3
    dense, funcs, contour, center, radius, F_node = _setup(engine, "dense", N, 2, True)
    terms3 = nc.random_terms(N, nterms, True)
    _install(engine, terms3, contour, nr.table([f for _, f in terms3], contour[0]))
    X = pc.random_block(N, m, 71)
    dX = engine.upload(X)
    dL = engine.upload(pc.random_block(2 * N, m, 73))          # a linearised block of the degree the handle's storage has
    lam = _points(center, radius, m)
    F = nr.table([f for _, f in terms3], lam)
    # every call that forms powers of lambda refuses a term handle and names the call to use
    powers = [lambda: engine.poly_solve(0.3 + 0.1j, dX, m), lambda: engine.poly_eval_cols(dX, lam, m), lambda: engine.poly_resinv_apply(dX, m),
              lambda: engine.poly_resinv_apply(dX, m, lam), lambda: engine.poly_ritz_eval(dX, m, np.eye(m), lam),
              lambda: engine.poly_contour_apply(dL, m), lambda: engine.poly_matmul(0, dL, m), lambda: engine.poly_project(dL, m),
              lambda: engine.poly_ritz_residual(dL, m, np.eye(m), lam, m)]
    for call in powers:
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "feasthip_nep_" in str(err.value)
    for solver in ("bicgstab", "cocg", "gmres"):
        with pytest.raises(FeastHipError) as err:
            engine.set_solver(solver)
        assert err.value.code == FPM_ERROR and "Krylov" in str(err.value)
    # the pencil entry points refuse it as they refuse a polynomial handle
    for call in (lambda: engine.orthonormalize(dX, m, 1e-8), lambda: engine.matmul(0, dX, m), lambda: engine.shifted_solve(0.3, dX, m)):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR
    # node values: wrong size, not finite, missing for the current contour
    with pytest.raises(FeastHipError) as err:
        engine.nep_set_node_values(nr.table([f for _, f in terms3], contour[0][:NE - 1]))
    assert err.value.code == FPM_ERROR
    badF = nr.table([f for _, f in terms3], contour[0])
    badF[3, 1] = np.nan
    with pytest.raises(FeastHipError) as err:
        engine.nep_set_node_values(badF)
    assert err.value.code == FPM_ERROR and "not finite" in str(err.value)
    other = fo.feast_gcontour(center + 0.1, radius, NE)
    engine.set_contour(other[0], other[1], 1.0)
    with pytest.raises(FeastHipError) as err:
        engine.nep_resinv_apply(dX, m)
    assert err.value.code == FPM_ERROR and "node values" in str(err.value)
    engine.set_contour(contour[0], contour[1], 1.0)
    assert not engine.nep_resinv_apply(dX, m)[1].any()
    # the table and the shifts go together; a table row that is not finite is refused
    with pytest.raises(FeastHipError) as err:
        engine.nep_resinv_apply(dX, m, lam, None)
    assert err.value.code == FPM_ERROR
    Fbad = F.copy()
    Fbad[2, 0] = np.inf
    with pytest.raises(FeastHipError) as err:
        engine.nep_resinv_apply(dX, m, lam, Fbad)
    assert err.value.code == FPM_ERROR and "not finite" in str(err.value)
    with pytest.raises(FeastHipError) as err:
        engine.nep_solve(NE, dX, m)
    assert err.value.code == FPM_ERROR
    with pytest.raises(FeastHipError) as err:
        engine.nep_resinv_apply(dX, 0)
    assert err.value.code == 2
    # a polynomial handle takes none of the nep calls
    engine.set_polynomial([A for A, _ in terms3])
    for call in (lambda: engine.nep_eval_cols(dX, F, m), lambda: engine.nep_resinv_apply(dX, m), lambda: engine.nep_solve(0, dX, m),
                 lambda: engine.nep_ritz_eval(dX, m, np.eye(m), F), lambda: engine.nep_set_node_values(nr.table([f for _, f in terms3], contour[0]))):
        with pytest.raises(FeastHipError) as err:
            call()
        assert err.value.code == FPM_ERROR and "term handle" in str(err.value)
    # nterms out of range
    with pytest.raises(FeastHipError) as err:
        engine.set_terms([np.eye(6)] * 10)
    assert err.value.code == FPM_ERROR


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_singular_node_gives_status_8(engine, restore, sparse):
    """T(z_0) = A_0 with an empty row: the factorisation of that node meets an exactly zero pivot"""
    N, m = 45, 3
    d = np.arange(1.0, N + 1)
    d[17] = 0.0
    A0, A1 = np.diag(d), np.eye(N)
    terms = [(sp.csr_matrix(A0) + 0.0 * sp.identity(N, format="csr"), 0), (sp.identity(N, format="csr"), 1)] if sparse else [(A0, 0), (A1, 1)]
    contour = fo.feast_gcontour(0.5, 0.3, NE)
    F = np.ones((NE, 2), dtype=np.complex128)
    F[0] = (1.0, 0.0)
    _install(engine, terms, contour, F)
    dX = engine.upload(pc.random_block(N, m, 79))
    _, code = engine.nep_solve(1, dX, m)
    assert code == 0
    try:
        _, code = engine.nep_solve(0, dX, m)
    except FeastHipError as err:          # (a rejected pivot of the multifrontal LU may come back as the call's own error)
        code = err.code
    assert code == 8
    if not sparse:
        _, status, _ = engine.nep_resinv_apply(dX, m)
        assert status[0] == 8 and not status[1:NE].any()


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def _fpm(fpm3=nc.FPM3, ne=nc.NE):
    fpm = fk.feastinit()
    fpm[8], fpm[3] = ne, fpm3
    return fpm


def _pinned(ref, again, fpm3=nc.FPM3):
    """the rule of polynomial_projected_reference: the restatement's history clears the threshold tenfold on both sides and its
    loop count survives a 1e-14 relative perturbation of the start block"""
    tol, L, h = 10.0 ** -fpm3, ref["loop"], ref["eps_history"]
    return h[L] <= tol / 10 and (L == 0 or h[L - 1] >= 10 * tol) and again["loop"] == L and again["info"] == 0


def _check(res, ref, again, terms, exact, ne=nc.NE):
    """a device run against the restatement's run on the same start block, the closed form and numpy on its vectors"""
    nep = res.stats["nonlinear"]
    dense, funcs = nr.split(terms)
    N = dense[0].shape[0]
    ref_err = nr.match_error(ref["lam"], exact) if ref["M"] == len(exact) else np.inf
    bound = max(10 * ref_err, 1e-12)
    lam_err = nr.match_error(res.lambda_, exact) if res.M == len(exact) else np.inf
    pinned = _pinned(ref, again)
    print("loop %d (restatement %d, %s) history %s (restatement %s) rank %s candidates %s set aside %s eigenvalue error %.2e (restatement %.2e, "
          "bound %.2e) factorizations %d" % (res.loop, ref["loop"], "pinned" if pinned else "not pinned", ["%.1e" % e for e in nep["eps_history"]],
                                            ["%.1e" % e for e in ref["eps_history"]], nep["rank"], nep["candidates"], nep["set_aside"], lam_err,
                                            ref_err, bound, res.stats["factorizations"]))
    assert ref["info"] == 0 and ref["M"] == len(exact)
    assert res.info == 0 and res.M == len(exact)
    assert lam_err <= bound
    assert res.loop == ref["loop"] if pinned else res.loop <= ref["loop"] + 1
    assert res.q.shape == (N, res.M) and np.abs(np.linalg.norm(res.q, axis=0) - 1.0).max() <= 16 * N * EPS
    be_np = nr.candidate_errors(dense, nr.table(funcs, res.lambda_), res.q)
    assert np.all(np.abs(be_np - res.res) <= 1e-3 * res.res + 16 * len(dense) * N * EPS)
    assert np.array_equal(nep["backward_error"], res.res) and res.epsout == res.res.max() == nep["eps_history"][-1] <= 1e-10
    assert np.all(np.diff(np.abs(res.lambda_) ** 2) >= 0)          # feast_sort_general order
    assert nep["terms"] == len(dense) and nep["moments"] == 2 and nep["reduced_nodes"] == 128
    assert len(nep["eps_history"]) == len(nep["rank"]) == len(nep["candidates"]) == len(nep["set_aside"]) == res.loop + 1
    assert res.stats["factorizations"] == ne and res.stats["solve_seconds"] > 0 and len(res.stats["ortho"]) == res.loop + 1


@pytest.mark.parametrize("N,circle", nc.DELAY_CASES, ids=nc.DELAY_IDS)
def test_driver_delay(engine, restore, N, circle):
    case = nc.delay_case(N, circle)
    for seed in nc.SEEDS if (N, circle) == (33, 2) else (1,):          # (the case with shared eigenvectors: every start seed)
        ref, again = nr.delay_run(N, circle, seed), nr.delay_run(N, circle, seed, perturb=1e-14)
        Q0 = fo.seeded_subspace(N, case["m0"], seed)
        res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0)
        _check(res, ref, again, case["terms"], case["lam_in"])
        assert res.stats["nonlinear"]["columns"] == case["m0"] and "plan" not in res.stats["nonlinear"]
    if circle == 0:
        rr = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0, ortho="cholqr_rr")
        assert rr.info == 0 and rr.M == case["count"] and nr.match_error(rr.lambda_, case["lam_in"]) <= 1e-7


@pytest.mark.parametrize("solver", ["sparse_direct", "direct"])
@pytest.mark.parametrize("dims", list(nc.GRID_CASES), ids=nc.GRID_IDS)
def test_driver_grid_delay(engine, restore, dims, solver):
    case = nc.grid_delay_case(dims)
    ref, again = nr.grid_run(dims, False, 1), nr.grid_run(dims, False, 1, perturb=1e-14)
    Q0 = fo.seeded_subspace(case["N"], case["m0"], 1)
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0, solver=solver)
    _check(res, ref, again, case["terms"], case["lam_in"])
    nep = res.stats["nonlinear"]
    if solver == "sparse_direct":
        assert nep["plan"] == "multifrontal" and nep["fell_back"] is False and "solver_substitution" not in res.stats
        assert nep["plan_nnz"] == len(polynomial_union_csr([A for A, _ in case["terms"]])[1]) and nep["plan_factor_bytes"] > 0 and nep["plan_flops"] > 0
    else:
        assert res.stats["solver_substitution"]["requested"] == "direct" and "plan" not in nep


@pytest.mark.parametrize("solver", ["sparse_direct", "direct"])
def test_driver_variable_coefficient(engine, restore, solver):
    """no closed form: the reference eigenvalues are the restatement's at a threshold of 1e-13, and the bound is ten times the
    error of the restatement's own run at 1e-10 against them"""
    dims = (6, 5, 4)
    case = nc.grid_delay_case(dims, True)
    m0 = nc.grid_delay_case(dims)["m0"]
    ref, again = nr.grid_run(dims, True, 1), nr.grid_run(dims, True, 1, perturb=1e-14)
    tight = nr.driver(case["terms"], case["center"], case["radius"], m0, seed=1, fpm3=13)
    assert tight["info"] == 0 and tight["M"] == ref["M"] > 0
    Q0 = fo.seeded_subspace(case["N"], m0, 1)
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=m0, fpm=_fpm(), engine=engine, Q0=Q0, solver=solver)
    _check(res, ref, again, case["terms"], tight["lam"])


def test_driver_rational(engine, restore):
    case = nc.rational_case()
    ref, again = nr.rational_run(1), nr.rational_run(1, perturb=1e-14)
    Q0 = fo.seeded_subspace(case["N"], case["m0"], 1)
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0)
    _check(res, ref, again, case["terms"], case["lam_in"])


@pytest.mark.parametrize("params", pc.DRIVER_CASES[:3], ids=pc.DRIVER_IDS[:3])
def test_driver_polynomial_posed_as_terms(engine, restore, params):
    N, d, k, _, monic = params
    case = nc.poly_as_terms(pc.make_case(N, d, k, monic))
    ref = nr.driver(case["terms"], case["center"], case["radius"], k + 2, seed=1)
    again = nr.driver(case["terms"], case["center"], case["radius"], k + 2, seed=1, perturb=1e-14)
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=k + 2, fpm=_fpm(), engine=engine, Q0=fo.seeded_subspace(N, k + 2, 1))
    _check(res, ref, again, case["terms"], case["lam_in"])


def test_driver_fallback_to_the_dense_expansion(engine, restore, monkeypatch):
    """the saddle-point quadratic of the polynomial tests posed as terms: the multifrontal LU rejects a pivot, the run repeats on
    the dense expansion"""
    monkeypatch.setenv("FH_MF_LEAF", "8")
    case = sc.saddle_quadratic()
    k = len(case["lam_in"])
    terms = [(A, p) for p, A in enumerate(case["coeffs"])]
    res = fk.feast_nonlinear(terms, case["center"], case["radius"], M0=k + 2, fpm=_fpm(sc.FPM3, sc.NE), engine=engine, solver="sparse_direct")
    nep = res.stats["nonlinear"]
    lam_err = nr.match_error(res.lambda_, case["lam_in"]) if res.M == k else np.inf
    print("M %d loop %d epsout %.2e eigenvalue error %.2e; %s" % (res.M, res.loop, res.epsout, lam_err, res.stats.get("solver_substitution")))
    assert nep["fell_back"] is True and nep["plan"] == "dense"
    assert res.stats["solver_substitution"]["requested"] == "sparse_direct" and "pivot" in res.stats["solver_substitution"]["reason"]
    assert res.info == 0 and res.M == k and res.epsout <= 1e-10 and lam_err <= 1e-8


def test_driver_empty_circle(engine, restore):
    N, circle = nc.EMPTY_CASE
    case = nc.delay_case(N, circle)
    assert case["count"] == 0
    res = fk.feast_nonlinear(case["terms"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine,
                             Q0=fo.seeded_subspace(N, case["m0"], 1))
    assert res.info == int(fk.FeastError.Feast_ERROR_NO_CONVERGENCE) and res.M == 0 and len(res.lambda_) == 0
    assert res.stats["factorizations"] == nc.NE


def test_driver_single_precision_keep_factors_and_loop_limit(engine, restore):
    N, circle = 40, 0
    case = nc.delay_case(N, circle)
    args = (case["center"], case["radius"])
    # float32 input: promoted, solved at the single-precision floor of the stop test (as in feast_polynomial), demoted.  The
    # reference is the restatement on the same rounded matrices with that floor as its threshold; the bound is ten times its own
    # error against the closed form of the unrounded problem (the rounding of the matrices moves the eigenvalues by about 1e-6)
    floor = float(np.sqrt(np.finfo(np.float32).eps))
    Q0 = fo.seeded_subspace(N, case["m0"], 1)
    single = [(A.astype(np.float32), f) for A, f in case["terms"]]
    ref = nr.driver([(A.astype(np.float64), f) for A, f in single], *args, case["m0"], seed=1, fpm3=-np.log10(floor))
    ref_err = nr.match_error(ref["lam"], case["lam_in"]) if ref["M"] == case["count"] else np.inf
    s = fk.feast_nonlinear(single, *args, M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0)
    s_err = nr.match_error(s.lambda_.astype(np.complex128), case["lam_in"]) if s.M == case["count"] else np.inf
    print("float32: M %d of %d loop %d (restatement %d) epsout %.2e eigenvalue error %.2e (restatement %.2e)" % (
        s.M, case["count"], s.loop, ref["loop"], s.epsout, s_err, ref_err))
    assert ref["info"] == 0 and s.info == 0 and s.M == case["count"] and s.lambda_.dtype == np.complex64 and s.q.dtype == np.complex64
    assert s.epsout <= floor and s_err <= max(10 * ref_err, 10 * np.finfo(np.float32).eps)
    # keep_factors: a second call on the same contour finds every node's factor
    a = fk.feast_nonlinear(case["terms"], *args, M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0, keep_factors=True)
    b = fk.feast_nonlinear(case["terms"], *args, M0=case["m0"], fpm=_fpm(), engine=engine, Q0=Q0)
    assert a.stats["factorizations"] == nc.NE and b.stats["factorizations"] == nc.NE          # (a new handle problem: the factors go with it)
    assert a.info == b.info == 0 and np.array_equal(a.lambda_, b.lambda_) and np.array_equal(a.q, b.q)
    # the loop limit returns the last iterates: the first case whose restatement is still a factor 100 above the threshold at loop 1
    Ns, cs = next(k for k in nc.DELAY_CASES if nr.delay_run(*k, 1)["loop"] >= 2 and nr.delay_run(*k, 1)["eps_history"][1] >= 1e-8)
    slow = nc.delay_case(Ns, cs)
    fpm = _fpm()
    fpm[4] = 1
    c = fk.feast_nonlinear(slow["terms"], slow["center"], slow["radius"], M0=slow["m0"], fpm=fpm, engine=engine, Q0=fo.seeded_subspace(Ns, slow["m0"], 1))
    assert c.info == int(fk.FeastError.Feast_ERROR_NO_CONVERGENCE) and c.loop == 1 and c.M > 0 and c.epsout > 1e-10
    # one moment loses the eigenvalues that share a vector, on the device as in the restatement
    shared = nc.delay_case(33, 2)
    one = fk.feast_nonlinear(shared["terms"], shared["center"], shared["radius"], M0=shared["m0"], fpm=_fpm(), engine=engine,
                             Q0=fo.seeded_subspace(33, shared["m0"], 1), moments=1)
    assert one.M < shared["count"]


def test_an_error_of_a_function_reaches_the_caller(engine, restore):
    """an f_k that fails where only the reduced solve evaluates it (the 128 nodes of Beyn's contour): its exception comes out
    of feast_nonlinear as it is, not as a LAPACK failure of the reduced problem"""
    case = nc.delay_case(33, 1)

    class Boom(RuntimeError):
        pass

    def f(z):
        if np.size(z) == 128:
            raise Boom("f_2 at the reduced nodes")
        return np.exp(-np.asarray(z, dtype=np.complex128))

    terms = list(case["terms"][:2]) + [(case["terms"][2][0], f)]
    with pytest.raises(Boom):
        fk.feast_nonlinear(terms, case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine)

    def g(z):
        return np.ones(3) if np.size(z) == 128 else np.exp(-np.asarray(z, dtype=np.complex128))

    with pytest.raises(ValueError, match="same shape"):
        fk.feast_nonlinear(list(case["terms"][:2]) + [(case["terms"][2][0], g)], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), engine=engine)
