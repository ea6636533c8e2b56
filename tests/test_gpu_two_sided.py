"""Two-sided FEAST on the device: the adjoint switch of the C ABI (conjugate-transposed substitution on the cached LU
factors, adjoint dense products and residual, oblique projection) against LAPACK / numpy, and the driver
feast_general(two_sided=True) against the prescribed spectra of tests/two_sided_cases.py and the host restatement."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import feastkit_jl_amd as fk
import two_sided_cases as tc
from feastkit_jl_amd.contour import feast_gcontour
from two_sided_reference import reference_run, residuals

pytestmark = pytest.mark.gpu

FPM_CODE = 9


def rand_block(N, m, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))


_pencils = {}


def pencil(N, cplx, with_B):
    """Non-symmetric A (real stored or complex) with its spectrum in the unit disc, optional general complex B; N = 839 is the
    unscaled complex Gaussian matrix of test_dense_lu_block_widths.  Built once per shape; read only."""
    key = (N, cplx, with_B)
    if key not in _pencils:
        rng = np.random.default_rng([N, int(cplx), int(with_B)])
        A = rng.standard_normal((N, N))
        if cplx:
            A = A + 1j * rng.standard_normal((N, N))
        if N != 839:
            A = A / np.sqrt(N)
        B = None
        if with_B:
            B = np.eye(N) + 0.3 * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) / np.sqrt(N)
        _pencils[key] = (np.asfortranarray(A), B)
    return _pencils[key]


@pytest.fixture
def adj(engine):
    """The session engine set up for the adjoint entry points; the switch is off again afterwards, whatever happened."""
    engine.set_real_projection(False)
    engine.set_solver("direct")
    engine.set_adjoint(False)
    yield engine
    engine.set_adjoint(False)


# ---- 1. adjoint shifted_solve against LAPACK 'C' -----------------------------------------------------------------------
SOLVE_SHAPES = [(N, m) for N in (96, 128, 130, 257, 839) for m in (5, 16, 40, 64)] + [(257, 80)]


@pytest.mark.parametrize("N,m", SOLVE_SHAPES)
@pytest.mark.parametrize("cplx,with_B", [(False, False), (True, False), (False, True), (True, True)])
def test_adjoint_shifted_solve(adj, N, m, cplx, with_B):
    """Bars of the forward solve: 1e-9 relative to LAPACK and residual 1e-11 (test_dense_lu_shifted_solve); 1e-8 and 1e-10 for
    the unscaled N = 839 Gaussian matrix (test_dense_lu_block_widths)."""
    A, B = pencil(N, cplx, with_B)
    adj.set_problem(A, B)
    z = 0.3 + 0.7j if N != 839 else 0.2 - 0.4j
    X = rand_block(N, m, 4)
    adj.set_adjoint(True)
    dY, rc = adj.shifted_solve(z, adj.upload(X), m)
    adj.set_adjoint(False)
    assert rc == 0
    Y = adj.download(dY)
    Sm = z * (np.eye(N) if B is None else B) - A
    ref = sla.lu_solve(sla.lu_factor(Sm), X, trans=2)
    err = np.abs(Y - ref).max() / np.abs(ref).max()
    res = (np.linalg.norm(Sm.conj().T @ Y - X, axis=0) / np.linalg.norm(X, axis=0)).max()
    print("N %d m %d err %.2e res %.2e" % (N, m, err, res))
    assert err <= (1e-8 if N == 839 else 1e-9)
    assert res < (1e-10 if N == 839 else 1e-11)


@pytest.mark.parametrize("kb,legacy_solve", [(64, False), (256, False), (128, True)])
def test_adjoint_solve_block_widths(kb, legacy_solve, monkeypatch):
    """The adjoint substitution reads the factor and the 128-block inverses, which every outer block width of the
    factorisation leaves in the same place, and never takes the 32-column steps: the handles of test_dense_lu_block_widths
    (FH_LU_KB, FH_LU_SOLVE_32; the environment is read when the handle is created), same matrix and bars."""
    monkeypatch.setenv("FH_LU_KB", str(kb))
    if legacy_solve:
        monkeypatch.setenv("FH_LU_SOLVE_32", "1")
    eng = fk.HipEngine(0)
    try:
        N, m = 839, 40
        A, _ = pencil(N, True, False)
        eng.set_problem(A, None)
        eng.set_solver("direct")
        z = 0.2 - 0.4j
        X = rand_block(N, m, 9)
        dX = eng.upload(X)
        dF, rc = eng.shifted_solve(z, dX, m)
        assert rc == 0 and eng.last_stats["factorizations"] == 1
        eng.set_adjoint(True)
        dY, rc = eng.shifted_solve(z, dX, m)
        assert rc == 0 and eng.last_stats["factorizations"] == 0
        Y = eng.download(dY)
        Sm = z * np.eye(N) - A
        assert (np.linalg.norm(Sm.conj().T @ Y - X, axis=0) / np.linalg.norm(X, axis=0)).max() < 1e-10
        ref = sla.lu_solve(sla.lu_factor(Sm), X, trans=2)
        assert np.abs(Y - ref).max() <= 1e-8 * np.abs(ref).max()
        assert (np.linalg.norm(Sm @ eng.download(dF) - X, axis=0) / np.linalg.norm(X, axis=0)).max() < 1e-10
    finally:
        eng.close()


# ---- 2. factor sharing -------------------------------------------------------------------------------------------------
def test_factor_sharing(adj):
    N, m = 257, 24
    A, B = pencil(N, True, True)
    adj.set_problem(A, B)
    z = -0.2 + 0.5j
    dX = adj.upload(rand_block(N, m, 5))
    out, nfact = [], []
    for on in (False, True, False, True):
        adj.set_adjoint(on)
        dY, rc = adj.shifted_solve(z, dX, m)
        assert rc == 0
        out.append(adj.download(dY))
        nfact.append(adj.last_stats["factorizations"])
    adj.set_adjoint(False)
    assert nfact == [1, 0, 0, 0]
    assert np.array_equal(out[0], out[2])
    assert np.array_equal(out[1], out[3])
    assert not np.array_equal(out[0], out[1])


# ---- 3. adjoint contour_apply ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,node_range", [(24, None), (24, (3, 4)), (80, None)])
def test_adjoint_contour_apply(adj, m, node_range):
    N, ne, scale = 257, 8, 1.0
    A, B = pencil(N, True, True)
    fpm = fk.feastinit()
    fpm[8] = ne
    fk.feastdefault(fpm)
    Zne, Wne = feast_gcontour(0.1 + 0.05j, 0.8, fpm)
    assert len(Zne) == ne
    adj.set_problem(A, B)
    adj.set_contour(Zne, Wne, scale)
    first, count = node_range if node_range else (0, ne)
    adj.set_node_range(first, count)
    Q = rand_block(N, m, 6)
    dQ = adj.upload(Q)
    _, status, st = adj.contour_apply(dQ, m)
    assert st["factorizations"] == count and not status[:count].any()
    adj.set_adjoint(True)
    dP, status, st = adj.contour_apply(dQ, m)
    adj.set_adjoint(False)
    adj.set_node_range(0, ne)
    assert st["factorizations"] == 0 and not status[:count].any()
    rhs = B.conj().T @ Q
    ref = sum(scale * np.conj(Wne[e]) * np.linalg.solve((Zne[e] * B - A).conj().T, rhs) for e in range(first, first + count))
    err = np.abs(adj.download(dP) - ref).max() / np.abs(ref).max()
    print("m %d nodes %s err %.2e" % (m, node_range, err))
    assert err <= 1e-9


# ---- 4. adjoint matmul -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [96, 130, 257, 1000])
@pytest.mark.parametrize("m", [1, 16, 33, 64])
@pytest.mark.parametrize("cplx", [False, True])
def test_adjoint_matmul(adj, N, m, cplx):
    """Bar of test_dense_matmul: 1e-11 relative to the largest entry."""
    rng = np.random.default_rng([N, int(cplx)])
    A = rng.standard_normal((N, N)) + (1j * rng.standard_normal((N, N)) if cplx else 0)
    B = rng.standard_normal((N, N)) + (1j * rng.standard_normal((N, N)) if cplx else 0)
    adj.set_problem(A, B)
    X = rand_block(N, m, 8)
    dX = adj.upload(X)
    adj.set_adjoint(True)
    YA = adj.download(adj.matmul(0, dX, m))
    YB = adj.download(adj.matmul(1, dX, m))
    adj.set_adjoint(False)
    refA, refB = A.conj().T @ X, B.conj().T @ X
    assert np.abs(YA - refA).max() <= 1e-11 * np.abs(refA).max()
    assert np.abs(YB - refB).max() <= 1e-11 * np.abs(refB).max()
    assert np.abs(adj.download(adj.matmul(0, dX, m)) - A @ X).max() <= 1e-11 * np.abs(refA).max()     # and off again


def test_adjoint_matmul_identity_B(adj):
    N, m = 130, 16
    A, _ = pencil(N, True, False)
    adj.set_problem(A, None)
    X = rand_block(N, m, 8)
    adj.set_adjoint(True)
    YB = adj.download(adj.matmul(1, adj.upload(X), m))
    adj.set_adjoint(False)
    assert np.abs(YB - X).max() <= 1e-11 * np.abs(X).max()


# ---- 5. project_pair and the adjoint ritz_residual ---------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(130, 16), (1000, 33)])
@pytest.mark.parametrize("with_B", [False, True])
def test_project_pair(adj, N, m, with_B):
    """Bar of test_project_matches_numpy: 1e-11 relative."""
    A, B = pencil(N, True, with_B)
    adj.set_problem(A, B)
    QL, QR = rand_block(N, m, 9), rand_block(N, m, 10)
    Aq, Bq = adj.project_pair(adj.upload(QL), adj.upload(QR), m)
    refA = QL.conj().T @ (A @ QR)
    refB = QL.conj().T @ (QR if B is None else B @ QR)
    assert np.abs(Aq - refA).max() <= 1e-11 * np.abs(refA).max()
    assert np.abs(Bq - refB).max() <= 1e-11 * np.abs(refB).max()


def test_project_ignores_the_switch(adj):
    """feasthip_project[_dev] applies A and B themselves with the switch on (narrow and 64-column-panel paths)."""
    N = 257
    A, B = pencil(N, True, True)
    adj.set_problem(A, B)
    for m in (24, 80):
        Q = rand_block(N, m, 13)
        dQ = adj.upload(Q)
        off = adj.project(dQ, m, bilinear=False, hermitize=False)
        adj.set_adjoint(True)
        on = adj.project(dQ, m, bilinear=False, hermitize=False)
        adj.set_adjoint(False)
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
        refA = Q.conj().T @ (A @ Q)
        assert np.abs(on[0] - refA).max() <= 1e-11 * np.abs(refA).max()


def test_project_pair_wide(adj):
    N, m = 257, 80
    A, B = pencil(N, True, True)
    adj.set_problem(A, B)
    QL, QR = rand_block(N, m, 9), rand_block(N, m, 10)
    adj.set_adjoint(True)                                   # independent of the switch
    Aq, Bq = adj.project_pair(adj.upload(QL), adj.upload(QR), m)
    adj.set_adjoint(False)
    refA, refB = QL.conj().T @ (A @ QR), QL.conj().T @ (B @ QR)
    assert np.abs(Aq - refA).max() <= 1e-11 * np.abs(refA).max()
    assert np.abs(Bq - refB).max() <= 1e-11 * np.abs(refB).max()


@pytest.mark.parametrize("N,r,M", [(130, 16, 9), (1000, 33, 33)])
@pytest.mark.parametrize("with_B,use_B", [(True, True), (True, False), (False, True)])
def test_adjoint_ritz_residual(adj, N, r, M, with_B, use_B):
    """Bars of test_ritz_residual: vectors 1e-11, residuals 1e-10 relative to the largest."""
    A, B = pencil(N, True, with_B)
    adj.set_problem(A, B)
    Q, V = rand_block(N, r, 2), rand_block(r, r, 3)
    lam = np.linspace(0.5, 3.0, r) * np.exp(1j * np.linspace(0.0, 2.0, r))
    adj.set_adjoint(True)
    dX, res = adj.ritz_residual(adj.upload(Q), r, V, lam, M, normalize=True, use_B=use_B)
    adj.set_adjoint(False)
    X = Q @ V
    X[:, :M] /= np.linalg.norm(X[:, :M], axis=0)
    assert np.abs(adj.download(dX) - X).max() <= 1e-11 * np.abs(X).max()
    BhX = X if (B is None or not use_B) else B.conj().T @ X
    R = A.conj().T @ X - BhX * np.conj(lam)[None, :]
    ref = np.linalg.norm(R[:, :M], axis=0) / np.maximum(np.abs(lam[:M]), 1.0)
    assert np.abs(res - ref).max() <= 1e-10 * ref.max()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(fk.FeastHipError) as ei:
        call()
    assert ei.value.code == FPM_CODE
    assert "adjoint" in str(ei.value) and len(str(ei.value)) > len("feasthip error 9: ")


def test_refusals_and_switch_off_is_bit_identical():
    eng = fk.HipEngine(0)
    try:
        N, m, ne = 130, 16, 8
        A, B = pencil(N, True, True)
        fpm = fk.feastinit()
        fpm[8] = ne
        fk.feastdefault(fpm)
        Zne, Wne = feast_gcontour(0.0, 0.9, fpm)
        eng.set_problem(A, B)
        eng.set_contour(Zne, Wne, 1.0)
        eng.set_node_range(0, ne)
        eng.set_solver("direct")
        dQ = eng.upload(rand_block(N, m, 11))
        before = eng.download(eng.contour_apply(dQ, m)[0])          # the switch has never been touched
        eng.set_adjoint(True)
        _refused(lambda: eng.contour_apply(dQ, m, want_moments=True))
        _refused(lambda: eng.contour_apply_resident(dQ, m))
        _refused(lambda: eng.estimate_count(m, 1))
        _refused(lambda: eng.rayleigh_ritz(dQ, m, -1.0, 1.0))
        eng.set_solver("direct", factor_precision=32)
        _refused(lambda: eng.contour_apply(dQ, m))
        _refused(lambda: eng.shifted_solve(0.3 + 0.1j, dQ, m))
        eng.set_solver("bicgstab")
        _refused(lambda: eng.contour_apply(dQ, m))
        eng.set_solver("direct")
        eng.set_real_projection(True)
        _refused(lambda: eng.contour_apply(dQ, m))
        eng.set_real_projection(False)
        adjoint = eng.download(eng.contour_apply(dQ, m)[0])
        eng.set_adjoint(False)
        after = eng.download(eng.contour_apply(dQ, m)[0])
        assert np.array_equal(before, after)
        assert not np.array_equal(before, adjoint)
    finally:
        eng.close()


def test_csr_problem_is_refused(adj):
    N, m = 200, 8
    A = sp.diags([np.full(N - 1, -1.0), np.full(N, 2.0), np.full(N - 1, -1.0)], [-1, 0, 1], format="csr")
    adj.set_problem(A, None)
    dX = adj.upload(rand_block(N, m, 12))
    adj.set_adjoint(True)
    _refused(lambda: adj.matmul(0, dX, m))
    _refused(lambda: adj.shifted_solve(0.3 + 0.1j, dX, m))
    adj.set_adjoint(False)
    assert np.abs(adj.download(adj.matmul(0, dX, m)) - A @ adj.download(dX)).max() <= 1e-12 * 4


# ---- 7. driver end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", tc.PARAMS, ids=tc.IDS)
def test_driver(adj, params):
    """Measured on one MI355X: see DESIGN.md section 6k."""
    case = tc.make_case(*params)
    ref = reference_run(params)
    A, B, n_in = case["A"], case["B"], case["n_in"]
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    res = fk.feast_general(A, B, tc.CENTER, tc.RADIUS, M0=case["M0"], fpm=fpm, engine=adj, two_sided=True)
    ts = res.stats["two_sided"]
    eps_dev = [max(a, b) for a, b in zip(ts["res_right"], ts["res_left"])]
    print("loops %d (restatement %d) epsout %.2e" % (res.loop, ref["loop"], res.epsout))
    print("epsout per loop, device     :", " ".join("%.1e" % e for e in eps_dev))
    print("epsout per loop, restatement:", " ".join("%.1e" % e for e in ref["eps_hist"]))
    assert res.M == n_in and res.info == 0
    assert np.abs(res.lambda_ - case["lam_in"]).max() <= 1e-10
    X, Y = res.q, res.q_left
    ny = np.linalg.norm(Y, axis=0)
    rr, rl = residuals(A, B, res.lambda_, X, Y / ny)
    print("host residuals: right %.2e left %.2e" % (rr.max(), rl.max()))
    assert rr.max() <= 1e-10 and rl.max() <= 1e-10
    assert ts["adjoint_factorizations"] == 0
    assert res.stats["factorizations"] == len(feast_gcontour(complex(tc.CENTER), tc.RADIUS, fpm)[0])
    BX = X if B is None else B @ X
    G = Y.conj().T @ BX
    assert np.abs(np.diag(G) - 1.0).max() <= 1e-12
    # (lam_i - lam_j) y_i^H B x_j = r_L,i^H x_j - y_i^H r_R,j for the residual VECTORS of the returned x_j (unit) and y_i (scaled):
    # ||r_R,j|| = rr_j max(|lam_j|, 1), ||r_L,i|| = rl_i max(|lam_i|, 1) ||y_i||; |lam_i - lam_j| >= the prescribed gap less the
    # 1e-10 the values may be off.  The fp64 evaluation of the inner product itself adds at most N eps ||y_i|| ||B x_j||.
    sc = np.maximum(np.abs(res.lambda_), 1.0)
    nrR, nrL = rr * sc, rl * sc * ny
    bound = (nrL[:, None] * np.linalg.norm(X, axis=0)[None, :] + ny[:, None] * nrR[None, :]) / (case["gap"] - 2e-10) \
        + case["N"] * np.finfo(float).eps * ny[:, None] * np.linalg.norm(BX, axis=0)[None, :]
    off = np.abs(G - np.diag(np.diag(G)))
    print("biorthogonality %.2e (reported %.2e), smallest bound %.2e" % (off.max(), ts["biorthogonality"], bound.min()))
    assert (off <= bound).all()
    assert abs(ts["biorthogonality"] - off.max()) <= 1e-13 + 1e-6 * off.max()
    for k in range(min(len(eps_dev), len(ref["eps_hist"]))):
        if eps_dev[k] > 1e-10 and ref["eps_hist"][k] > 1e-10:
            assert ref["eps_hist"][k] / 10 <= eps_dev[k] <= ref["eps_hist"][k] * 10, k
    assert res.loop <= ref["loop"] + 1
    assert np.abs(ts["overlap"] - case["overlap"]).max() <= 1e-8 * case["overlap"].max()
    assert (np.abs(ts["overlap"] - case["overlap"]) <= 1e-8 * case["overlap"]).all()


# ---- 8. the one-sided call is unchanged --------------------------------------------------------------------------------
def test_one_sided_call_has_no_left_vectors(adj):
    case = tc.make_case(*tc.PARAMS[0])
    assert case["N"] == 96 and case["B"] is None
    res = fk.feast_general(case["A"], None, 0, 1, M0=12, engine=adj)
    assert res.q_left is None and "two_sided" not in res.stats
