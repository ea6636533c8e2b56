"""Two-sided FEAST on sparse input, on the device: the adjoint switch of the C ABI on a CSR problem under the sparse direct
solver's multifrontal plan (conjugate-transposed walk through the front tree on the cached factors, products on the
conjugate-transposed CSR set) against SuperLU / scipy, and the driver feast_general(A_sparse, ..., two_sided=True) against
scipy.linalg.eigvals and the host restatement on the cases of tests/two_sided_sparse_cases.py."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feastkit_jl_amd as fk
import two_sided_sparse_cases as sc
from feastkit_jl_amd import workloads
from feastkit_jl_amd.contour import feast_gcontour
from test_gpu_multifrontal import grid_pencil
from test_gpu_wband import random_pencil
from two_sided_reference import residuals

pytestmark = pytest.mark.gpu

FPM_CODE = 9


def rand_block(N, m, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))


@pytest.fixture
def force_mf(monkeypatch):
    monkeypatch.setenv("FH_MF", "1")


@pytest.fixture
def adj(engine):
    """The session engine set up for the adjoint entry points on CSR problems; both switches are off again afterwards."""
    engine.set_real_projection(False)
    engine.set_solver("banded")
    engine.set_adjoint(False)
    engine.require_adjoint(False)
    yield engine
    engine.set_adjoint(False)
    engine.require_adjoint(False)


def check_adjoint_solve(engine, A, B, z, m, seed=5, tol=2e-10):
    """check_solve of tests/test_gpu_wband.py for S^H Y = X: same bars, SuperLU's trans='H' as the reference."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
    engine.set_adjoint(True)
    try:
        dY, rc = engine.shifted_solve(z, engine.upload(X), m)
    finally:
        engine.set_adjoint(False)
    assert rc == 0
    Y = engine.download(dY, m)
    S = (z * (B if B is not None else sp.identity(n)) - A).tocsc().astype(complex)
    SH = S.conj().T.tocsr()
    ref = spla.splu(S).solve(X, trans="H")
    res = np.linalg.norm(SH @ Y - X) / np.linalg.norm(X)
    res_ref = np.linalg.norm(SH @ ref - X) / np.linalg.norm(X)
    print("n %d m %d residual %.2e (SuperLU %.2e) err %.2e" % (n, m, res, res_ref, np.abs(Y - ref).max() / np.abs(ref).max()))
    assert res <= max(tol, 50 * res_ref), (res, res_ref)
    assert np.abs(Y - ref).max() <= 1e-6 * np.abs(ref).max()
    return Y


# ---- 1. adjoint shifted_solve against SuperLU 'H' ----------------------------------------------------------------------
@pytest.mark.parametrize("shape,m,cplx,unsym,leaf,with_B", [
    ((6, 5, 4), 5, False, False, None, True),          # smallest tree
    ((12, 10, 8), 16, True, False, None, True),
    ((20, 16, 9), 64, False, True, None, True),
    ((25, 20, 12), 33, True, True, "24", True),        # deep tree
    ((30, 30, 1), 40, False, False, "200", True),      # 2-D, large leaves
    ((34, 26, 12), 64, False, False, None, True),      # groups with 128-block inverses
    ((12, 10, 8), 80, True, False, None, True),        # 64-column panels
    ((20, 16, 9), 64, False, True, None, False),       # identity B
])
def test_adjoint_solve_matches_superlu(adj, force_mf, monkeypatch, shape, m, cplx, unsym, leaf, with_B):
    if leaf:
        monkeypatch.setenv("FH_MF_LEAF", leaf)
    A, B = grid_pencil(*shape, seed=sum(shape) + min(m, 64), cplx=cplx, unsym=unsym)
    if not with_B:
        B = None
    adj.set_problem(A, B)
    adj.set_solver("banded")
    assert adj.band_plan()[3] == 2
    check_adjoint_solve(adj, A, B, 0.3 + 0.8j, m)
    check_adjoint_solve(adj, A, B, -0.4 + 0.3j, m, seed=9)         # a second shift through the cached-slot logic
    assert adj.band_plan()[3] == 2


def test_adjoint_solve_random_pattern(adj, force_mf):
    A, B = random_pencil(500, 40, 0.3, 23 + 500, True, False)      # unsymmetric PATTERN: the plan works on pattern U pattern^T
    adj.set_problem(A, B)
    adj.set_solver("banded")
    assert adj.band_plan()[3] == 2
    check_adjoint_solve(adj, A, B, 0.3 + 0.8j, 16)
    assert adj.band_plan()[3] == 2


# ---- 2. factor sharing and reproducibility -----------------------------------------------------------------------------
def test_factor_sharing_and_reproducibility(adj, force_mf):
    A, B = grid_pencil(12, 10, 8, seed=77, cplx=True, unsym=True)
    n, m = A.shape[0], 24
    adj.set_problem(A, B)
    adj.set_solver("banded")
    adj.free_factors()
    assert adj.band_plan()[3] == 2
    z = -0.2 + 0.5j
    dX = adj.upload(rand_block(n, m, 5))
    out, nfact = [], []
    for on in (False, True, False, True):
        adj.set_adjoint(on)
        dY, rc = adj.shifted_solve(z, dX, m)
        assert rc == 0
        out.append(adj.download(dY, m))
        nfact.append(adj.last_stats["factorizations"])
    assert nfact == [1, 0, 0, 0]
    assert np.array_equal(out[0], out[2])
    assert np.array_equal(out[1], out[3])
    assert not np.array_equal(out[0], out[1])
    adj.free_factors()
    adj.set_adjoint(True)
    dY, rc = adj.shifted_solve(z, dX, m)
    adj.set_adjoint(False)
    assert rc == 0 and adj.last_stats["factorizations"] == 1
    assert np.array_equal(adj.download(dY, m), out[1])


def skew_pencil():
    """laplacian_3d_pencil(12, 10, 8) made non-symmetric by a skew random term on the stencil's off-diagonal pattern."""
    A, B, _ = workloads.laplacian_3d_pencil(12, 10, 8)
    A = sp.csr_matrix(A)
    rng = np.random.default_rng(31)
    K = sp.triu(A, k=1).tocsr()
    K.data = 0.3 * rng.standard_normal(K.nnz)
    return (A + K - K.T).tocsr(), sp.csr_matrix(B)


def _contour(ne, center, radius):
    fpm = fk.feastinit()
    fpm[8] = ne
    fk.feastdefault(fpm)
    Zne, Wne = feast_gcontour(center, radius, fpm)
    assert len(Zne) == ne
    return Zne, Wne


def test_adjoint_contour_apply_node_batches_same_bits(adj, force_mf, monkeypatch):
    A, B = skew_pencil()
    n, m, ne = A.shape[0], 24, 8
    Zne, Wne = _contour(ne, 0.4 + 0.1j, 0.3)
    adj.set_problem(A, B)
    adj.set_contour(Zne, Wne, 1.0)
    adj.set_node_range(0, ne)
    adj.set_solver("banded")
    dQ = adj.upload(rand_block(n, m, 6))
    adj.set_adjoint(True)
    try:
        got = adj.download(adj.contour_apply(dQ, m)[0], m)
        monkeypatch.setenv("FH_MF_NODES_PER_CALL", "3")
        adj.free_factors()
        dP, status, st = adj.contour_apply(dQ, m)
    finally:
        adj.set_adjoint(False)
    assert st["factorizations"] == ne and not status[:ne].any()
    assert np.array_equal(adj.download(dP, m), got)


# ---- 3. adjoint contour_apply ------------------------------------------------------------------------------------------
_contour_refs = {}


def _contour_reference(A, B, Zne, Wne, Q, nodes):
    key = (Q.shape[1], nodes)
    if key not in _contour_refs:
        rhs = B.conj().T @ Q
        _contour_refs[key] = sum(np.conj(Wne[e]) * spla.splu((Zne[e] * B - A).tocsc().astype(complex)).solve(rhs, trans="H") for e in range(*nodes))
    return _contour_refs[key]


@pytest.mark.parametrize("m,node_range", [(24, None), (24, (3, 4)), (80, None)])
def test_adjoint_contour_apply(adj, force_mf, m, node_range):
    """Bar of the dense twin (tests/test_gpu_two_sided.py): 1e-9 relative."""
    A, B = skew_pencil()
    n, ne = A.shape[0], 8
    Zne, Wne = _contour(ne, 0.4 + 0.1j, 0.3)
    adj.set_problem(A, B)
    adj.set_contour(Zne, Wne, 1.0)
    first, count = node_range if node_range else (0, ne)
    adj.set_node_range(first, count)
    adj.set_solver("banded")
    adj.free_factors()
    assert adj.band_plan()[3] == 2
    Q = rand_block(n, m, 6)
    dQ = adj.upload(Q)
    try:
        _, status, st = adj.contour_apply(dQ, m)
        assert st["factorizations"] == count and not status[:count].any()
        adj.set_adjoint(True)
        dP, status, st = adj.contour_apply(dQ, m)
    finally:
        adj.set_adjoint(False)
        adj.set_node_range(0, ne)
    assert st["factorizations"] == 0 and not status[:count].any()
    ref = _contour_reference(A, B, Zne, Wne, Q, (first, first + count))
    err = np.abs(adj.download(dP, m) - ref).max() / np.abs(ref).max()
    print("m %d nodes %s err %.2e" % (m, node_range, err))
    assert err <= 1e-9


# ---- 4. adjoint matmul and ritz_residual on CSR ------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 16, 33, 64])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("with_B", [True, False])
def test_adjoint_matmul_and_residual_csr(adj, force_mf, m, cplx, with_B):
    """Bars of tests/test_gpu_two_sided.py: products 1e-11, residuals 1e-10, relative to the largest entry."""
    A, B = grid_pencil(9, 8, 7, seed=40 + int(cplx), cplx=cplx, unsym=True)           # N = 504
    if not with_B:
        B = None
    n = A.shape[0]
    adj.set_problem(A, B)
    adj.set_solver("banded")
    assert adj.band_plan()[3] == 2
    X = rand_block(n, m, 8)
    dX = adj.upload(X)
    forward_before = adj.download(adj.matmul(0, dX, m), m)
    V = rand_block(m, m, 3)
    lam = np.linspace(0.5, 3.0, m) * np.exp(1j * np.linspace(0.0, 2.0, m))
    adj.set_adjoint(True)
    try:
        YA = adj.download(adj.matmul(0, dX, m), m)
        YB = adj.download(adj.matmul(1, dX, m), m)
        dR, res = adj.ritz_residual(dX, m, V, lam, m, normalize=True, use_B=True)
    finally:
        adj.set_adjoint(False)
    AH = A.conj().T.tocsr()
    refA = AH @ X
    refB = X if B is None else B.conj().T @ X
    assert np.abs(YA - refA).max() <= 1e-11 * np.abs(refA).max()
    assert np.abs(YB - refB).max() <= 1e-11 * np.abs(refB).max()
    XV = X @ V
    XV /= np.linalg.norm(XV, axis=0)
    assert np.abs(adj.download(dR, m) - XV).max() <= 1e-11 * np.abs(XV).max()
    R = AH @ XV - (XV if B is None else B.conj().T @ XV) * np.conj(lam)[None, :]
    ref = np.linalg.norm(R, axis=0) / np.maximum(np.abs(lam), 1.0)
    assert np.abs(res - ref).max() <= 1e-10 * ref.max()
    forward_after = adj.download(adj.matmul(0, dX, m), m)                                # and off again: unchanged
    assert np.array_equal(forward_before, forward_after)
    assert np.abs(forward_after - A @ X).max() <= 1e-11 * np.abs(refA).max()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _refused(call, word=None):
    with pytest.raises(fk.FeastHipError) as ei:
        call()
    assert ei.value.code == FPM_CODE
    assert "adjoint" in str(ei.value) and len(str(ei.value)) > len("feasthip error 9: ")
    if word:
        assert word in str(ei.value)


def test_refusals_on_csr(force_mf):
    eng = fk.HipEngine(0)
    try:
        A, B = grid_pencil(6, 5, 4, seed=3, cplx=True, unsym=True)
        n, m, ne = A.shape[0], 8, 8
        Zne, Wne = _contour(ne, 0.2 + 0.1j, 0.6)
        eng.set_problem(A, B)
        eng.set_contour(Zne, Wne, 1.0)
        eng.set_node_range(0, ne)
        eng.set_solver("banded")
        dQ = eng.upload(rand_block(n, m, 11))
        before = eng.download(eng.contour_apply(dQ, m)[0], m)
        eng.set_adjoint(True)
        _refused(lambda: eng.contour_apply(dQ, m, want_moments=True))
        _refused(lambda: eng.contour_apply_resident(dQ, m))
        _refused(lambda: eng.estimate_count(m, 1))
        eng.set_solver("bicgstab")
        _refused(lambda: eng.contour_apply(dQ, m))
        _refused(lambda: eng.shifted_solve(0.3 + 0.1j, dQ, m))
        _refused(lambda: eng.matmul(0, dQ, m))
        eng.set_solver("direct")
        _refused(lambda: eng.shifted_solve(0.3 + 0.1j, dQ, m))
        eng.set_solver("banded", factor_precision=32)
        _refused(lambda: eng.contour_apply(dQ, m))
        _refused(lambda: eng.shifted_solve(0.3 + 0.1j, dQ, m))
        eng.set_solver("banded")
        eng.set_real_projection(True)
        _refused(lambda: eng.contour_apply(dQ, m))
        eng.set_real_projection(False)
        adjoint = eng.download(eng.contour_apply(dQ, m)[0], m)
        eng.set_adjoint(False)
        after = eng.download(eng.contour_apply(dQ, m)[0], m)
        assert np.array_equal(before, after)
        assert not np.array_equal(before, adjoint)
    finally:
        eng.close()


def test_band_plan_is_refused_until_required(monkeypatch):
    """A tridiagonal matrix takes the narrow band LU (plan 1), which has no adjoint form: refused with the plan named; with
    require_adjoint the same matrix takes the multifrontal plan and the adjoint solve meets the bars of check_solve."""
    monkeypatch.delenv("FH_MF", raising=False)
    monkeypatch.delenv("FH_WBAND", raising=False)
    eng = fk.HipEngine(0)
    try:
        N, m = 200, 8
        rng = np.random.default_rng(17)
        A = sp.diags([0.5 * rng.standard_normal(N - 1), 2.0 + 0.5 * rng.standard_normal(N), 0.5 * rng.standard_normal(N - 1)], [-1, 0, 1], format="csr")
        eng.set_problem(A, None)
        eng.set_solver("banded")
        assert eng.band_plan()[3] == 0
        dX = eng.upload(rand_block(N, m, 12))
        eng.set_adjoint(True)
        _refused(lambda: eng.shifted_solve(0.3 + 0.1j, dX, m), "plan 1")
        _refused(lambda: eng.matmul(0, dX, m), "plan 1")
        eng.set_adjoint(False)
        eng.require_adjoint(True)
        assert eng.band_plan()[3] == 2
        check_adjoint_solve(eng, A, None, 0.3 + 0.8j, m)
        assert eng.band_plan()[3] == 2
        eng.require_adjoint(False)
        assert eng.band_plan()[3] == 0                 # the calls that never asked keep the plan they had
    finally:
        eng.close()


# ---- 6. driver end to end ----------------------------------------------------------------------------------------------
def _match(lam, want):
    """index of the nearest entry of `want` for every computed value; must be a bijection"""
    idx = np.argmin(np.abs(lam[:, None] - want[None, :]), axis=1)
    assert len(set(idx.tolist())) == len(want) == len(lam)
    return idx


def _check_driver(res, case, ref, fpm):
    A, B, k = case["A"], case["B"], case["k"]
    ts = res.stats["two_sided"]
    eps_dev = [max(a, b) for a, b in zip(ts["res_right"], ts["res_left"])]
    print("loops %d (restatement %d) epsout %.2e plan %s" % (res.loop, ref["loop"], res.epsout, ts["direct_plan"]))
    print("epsout per loop, device     :", " ".join("%.1e" % e for e in eps_dev))
    print("epsout per loop, restatement:", " ".join("%.1e" % e for e in ref["eps_hist"]))
    assert res.M == k and res.info == 0
    idx = _match(res.lambda_, case["lam_in"])
    assert np.abs(res.lambda_ - case["lam_in"][idx]).max() <= 1e-10
    X, Y = res.q, res.q_left
    Ac = A.astype(complex)
    Bc = None if B is None else B.astype(complex)
    rr, rl = residuals(Ac, Bc, res.lambda_, X, Y / np.linalg.norm(Y, axis=0))
    print("host residuals: right %.2e left %.2e" % (rr.max(), rl.max()))
    assert rr.max() <= 1e-10 and rl.max() <= 1e-10
    G = Y.conj().T @ (X if B is None else B @ X)
    assert np.abs(np.diag(G) - 1.0).max() <= 1e-12
    assert ts["adjoint_factorizations"] == 0
    assert res.stats["factorizations"] == len(feast_gcontour(case["center"], case["radius"], fpm)[0])
    ridx = _match(res.lambda_, ref["lam"])
    print("overlap device", ts["overlap"], "restatement", ref["overlap"][ridx])
    assert (np.abs(ts["overlap"] - ref["overlap"][ridx]) <= 1e-8 * ref["overlap"][ridx]).all()
    assert res.loop <= ref["loop"] + 2
    for j in range(min(len(eps_dev), len(ref["eps_hist"]))):
        if 1e-10 < eps_dev[j] < 1e-2 and 1e-10 < ref["eps_hist"][j] < 1e-2:
            assert ref["eps_hist"][j] / 10 <= eps_dev[j] <= ref["eps_hist"][j] * 10, j


@pytest.mark.parametrize("params", sc.PARAMS, ids=sc.IDS)
def test_driver_sparse_direct(adj, params):
    """Measured on one MI355X: see DESIGN.md section 6l."""
    case = sc.make_case(*params)
    ref = sc.reference_run(params)
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    res = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], M0=case["M0"], fpm=fpm, engine=adj, two_sided=True,
                           solver="sparse_direct")
    assert res.stats["two_sided"]["direct_plan"].startswith("multifrontal")
    _check_driver(res, case, ref, fpm)


def test_driver_default_solver_takes_the_dense_substitution(adj):
    params = sc.PARAMS[2]
    case = sc.make_case(*params)
    assert case["N"] == 504
    ref = sc.reference_run(params)
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    res = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], M0=case["M0"], fpm=fpm, engine=adj, two_sided=True)
    assert "dense" in res.stats["solver_substitution"]["used"] and res.stats["two_sided"]["direct_plan"] == "dense LU"
    _check_driver(res, case, ref, fpm)


# ---- 7. the one-sided call is unchanged --------------------------------------------------------------------------------
def test_one_sided_call_unchanged():
    case = sc.make_case(*sc.PARAMS[1])
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    kw = dict(M0=case["M0"], fpm=fpm, solver="sparse_direct")
    eng = fk.HipEngine(0)
    try:
        before = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, **kw)      # require_adjoint never touched
        two = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, two_sided=True, **kw)
        after = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, **kw)
    finally:
        eng.close()
    assert two.q_left is not None and two.info == 0
    assert before.q_left is None and after.q_left is None and "two_sided" not in after.stats
    assert before.M == after.M == case["k"] and before.loop == after.loop
    assert np.array_equal(before.lambda_, after.lambda_) and np.array_equal(before.q, after.q) and np.array_equal(before.res, after.res)
