"""The adjoint substitution of the blocked band LU (fh_wband_solve_adjoint: ZGBTRS 'C' on the factors of fh_wband_factor) and
two-sided FEAST on the pencils that only the band LU factors: what feasthip_require_adjoint gives when the multifrontal LU
rejects a pivot, or is made to (FH_MF_MAX_MULTIPLIER=0 rejects every matrix: the deterministic way to the band plan on
well-conditioned input).  Bars are those of the multifrontal adjoint (tests/test_gpu_two_sided_sparse.py) and of the one-sided
pivoting tests (tests/test_gpu_direct_pivoting.py), imported where they exist as functions."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feastkit_jl_amd as fk
import two_sided_sparse_cases as sc
from test_gpu_direct_pivoting import BAND, MF, _finite_eigs_near, cond1, load, oseen_pencil, random_zero_diagonal
from test_gpu_multifrontal import grid_pencil
from test_gpu_two_sided_sparse import _check_driver, _contour, _match, check_adjoint_solve, rand_block, skew_pencil
from test_gpu_wband import check_solve, random_pencil
from two_sided_reference import two_sided_reference

pytestmark = pytest.mark.gpu


@pytest.fixture
def own_plan(monkeypatch):
    for v in ("FH_MF", "FH_MF_LEAF", "FH_WBAND", "FH_MF_MAX_MULTIPLIER", "FH_MF_NODES_PER_CALL"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture
def reject_all(monkeypatch, own_plan):
    monkeypatch.setenv("FH_MF_MAX_MULTIPLIER", "0")


@pytest.fixture
def adj(engine):
    """The session engine under the sparse direct solver with both adjoint switches off, before and after."""
    engine.set_real_projection(False)
    engine.set_solver("banded")
    engine.set_adjoint(False)
    engine.require_adjoint(False)
    yield engine
    engine.set_adjoint(False)
    engine.require_adjoint(False)
    engine._problem_fp = None                # the next set_problem makes its own plan, whatever a fallback left here


def tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    return sp.diags([0.5 * rng.standard_normal(n - 1), 2.0 + 0.5 * rng.standard_normal(n), 0.5 * rng.standard_normal(n - 1)],
                    [-1, 0, 1], format="csr")


def _complex_B(A, seed):
    """a complex upper-bidiagonal B: well conditioned, neither Hermitian nor symmetric"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    return (sp.diags(1.0 + 0.2 * rng.random(n) + 0.1j * rng.standard_normal(n)) +
            sp.diags(0.05 * (rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)), 1)).tocsr()


# ---- 1. adjoint shifted_solve on the band plan against SuperLU 'H' -------------------------------------------------------------
def _grid(shape, cplx, unsym, with_B):
    A, B = grid_pencil(*shape, seed=sum(shape) + 7, cplx=cplx, unsym=unsym)
    return A, (B if with_B else None)


SOLVE_CASES = {
    # N = 120 < one 128-block: a single partial block, ragged columns
    "one-partial-block-m5": (lambda: _grid((6, 5, 4), False, False, True), 5),
    # N = 960: several blocks, kl < 128
    "blocks-kl-lt-128-m16": (lambda: _grid((12, 10, 8), True, False, True), 16),
    # N = 2880, kl > 128 after reverse Cuthill-McKee: the left-looking update takes several chunks of k per wave
    "kl-gt-128-m64": (lambda: _grid((20, 16, 9), False, True, True), 64),
    "kl-gt-128-m80": (lambda: _grid((20, 16, 9), False, True, True), 80),           # two 64-column panels
    "identity-B-m33": (lambda: _grid((12, 10, 8), False, True, False), 33),
    "complex-B-m16": (lambda: (lambda A: (A, _complex_B(A, 4)))(_grid((12, 10, 8), True, True, True)[0]), 16),
    "unsymmetric-pattern-m16": (lambda: random_pencil(500, 40, 0.3, 23 + 500, True, False), 16),
    # kl = ku = 1, N = 2 x 128 + 1: a last block of one row
    "tridiagonal-257-m8": (lambda: (tridiagonal(257, 17), None), 8),
}


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
def test_adjoint_solve_on_band_plan_matches_superlu(adj, reject_all, name):
    make, m = SOLVE_CASES[name]
    A, B = make()
    adj.require_adjoint(True)
    load(adj, A, B)
    adj.set_solver("banded")
    assert adj.band_plan()[3] == MF                  # the requirement plans the multifrontal LU; its first factorisation is rejected
    check_adjoint_solve(adj, A, B, 0.3 + 0.8j, m)
    assert adj.band_plan()[3] == BAND
    kl, ku = adj.band_plan()[:2]
    print("%s: N %d band kl %d ku %d" % (name, A.shape[0], kl, ku))
    if name.startswith("kl-gt-128"):
        assert kl > 128
    check_adjoint_solve(adj, A, B, -0.4 + 0.3j, m, seed=9)           # a second shift through the cached-slot logic
    assert adj.band_plan()[3] == BAND                # kept while the requirement is on: no re-planning
    # ... and the forward solve on the same plan still meets its bar with the switch off again
    check_solve(adj, A, B, -0.4 + 0.3j, m, seed=9)
    assert adj.last_stats["factorizations"] == 0


# ---- 2. pivoting exercised -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [1e-5j, 0.3 + 0.2j])
@pytest.mark.parametrize("cplx", [False, True])
def test_adjoint_solve_zero_diagonal(adj, reject_all, cplx, z):
    """strict_solve of tests/test_gpu_direct_pivoting.py, transposed: S^H Y = X against SuperLU trans='H', residual <= max(1e-12,
    50 x SuperLU's), elementwise error relative to max|ref| under max(1e-12, 1e-13 cond_1).  The exactly zero diagonal gives
    interchanges in every block column, across block boundaries (N = 300: three blocks)."""
    A = random_zero_diagonal(300, 6, 0.5, 21 + cplx, cplx)
    n, m = A.shape[0], 12
    adj.require_adjoint(True)
    load(adj, A, None)
    adj.set_solver("banded")
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
    S = (z * sp.identity(n) - A).tocsc().astype(complex)
    lu = spla.splu(S)
    cond = cond1(lu, n) * spla.onenormest(S)
    want = lu.solve(X, trans="H")
    adj.set_adjoint(True)
    try:
        dY, rc = adj.shifted_solve(z, adj.upload(X), m)
    finally:
        adj.set_adjoint(False)
    Y = adj.download(dY, m)
    SH = S.conj().T.tocsr()
    res = np.linalg.norm(SH @ Y - X) / np.linalg.norm(X)
    res_ref = np.linalg.norm(SH @ want - X) / np.linalg.norm(X)
    err = np.abs(Y - want).max() / np.abs(want).max()
    msg = f"z={z} rc={rc} plan {adj.band_plan()[3]} residual {res:.2e} (SuperLU {res_ref:.2e}) error {err:.2e} cond {cond:.1e}"
    print(msg)
    assert rc == 0, msg
    assert adj.band_plan()[3] == BAND, msg
    assert res <= max(1e-12, 50 * res_ref), msg
    assert err <= max(1e-12, 1e-13 * cond), msg


# ---- 3. forward bits untouched, factors shared -----------------------------------------------------------------------------------
def test_forward_bits_untouched_and_factors_shared(adj, reject_all):
    A, B = skew_pencil()
    n, m, ne = A.shape[0], 24, 8
    Zne, Wne = _contour(ne, 0.4 + 0.1j, 0.3)
    adj.require_adjoint(True)
    load(adj, A, B)
    adj.set_contour(Zne, Wne, 1.0)
    adj.set_node_range(0, ne)
    adj.set_solver("banded")
    Q = rand_block(n, m, 6)
    dQ = adj.upload(Q)
    try:
        dP, status, st = adj.contour_apply(dQ, m)
        assert st["factorizations"] == ne and not status[:ne].any()
        assert adj.band_plan()[3] == BAND
        forward = adj.download(dP, m)
        adj.set_adjoint(True)
        dP, status, st = adj.contour_apply(dQ, m)
        assert st["factorizations"] == 0 and not status[:ne].any()
        adjoint = adj.download(dP, m)
        dP, status, st = adj.contour_apply(dQ, m)
        assert st["factorizations"] == 0
        adjoint_again = adj.download(dP, m)
        adj.set_adjoint(False)
        dP, status, st = adj.contour_apply(dQ, m)
        assert st["factorizations"] == 0 and not status[:ne].any()
        forward_again = adj.download(dP, m)
    finally:
        adj.set_adjoint(False)
    assert adj.band_plan()[3] == BAND
    assert np.array_equal(forward, forward_again)
    assert np.array_equal(adjoint, adjoint_again)
    rhs = B.conj().T @ Q
    ref = sum(np.conj(Wne[e]) * spla.splu((Zne[e] * B - A).tocsc().astype(complex)).solve(rhs, trans="H") for e in range(ne))
    err = np.abs(adjoint - ref).max() / np.abs(ref).max()
    print("adjoint contour_apply on band factors: err %.2e" % err)
    assert err <= 1e-9


# ---- 4. driver on forced fallback ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", sc.PARAMS, ids=sc.IDS)
def test_driver_on_forced_fallback(adj, reject_all, params):
    case = sc.make_case(*params)
    ref = sc.reference_run(params)
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    adj._problem_fp = None                   # a fresh plan: the fallback is seen by this call
    res = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], M0=case["M0"], fpm=fpm, engine=adj, two_sided=True,
                           solver="sparse_direct")
    assert res.info == 0, (res.info, res.stats)
    ts = res.stats["two_sided"]
    assert ts["direct_plan"].startswith("band LU") and ts["fell_back"] is True
    _check_driver(res, case, ref, fpm)


# ---- 5. driver on a pencil the multifrontal plan rejects by itself ----------------------------------------------------------------
def test_driver_saddle_point_two_sided(adj, own_plan, monkeypatch):
    """the interleaved 45 x 45 Oseen pencil and the circle rule of test_feast_general_saddle_point, two-sided: exactly singular
    leaf blocks hand the matrix to the band LU inside the first sweep, and the left sweep runs on those factors"""
    monkeypatch.setenv("FH_MF", "1")
    nx = ny = 45
    A, B = oseen_pencil(nx, ny, 17)
    order = []
    for i in range(nx):
        for j in range(ny):
            order.append(i * ny + j)
            if i < nx - 1 and j < ny - 1:
                order.append(nx * ny + i * (ny - 1) + j)
    order = np.asarray(order)
    A, B = A[order][:, order].tocsr(), B[order][:, order].tocsr()
    adj._problem_fp = None
    center = 2.0 + 0.0j
    lam = _finite_eigs_near(A, B, center, 30)
    d = np.abs(lam - center)
    k = 8 + int(np.argmax(d[9:20] - d[8:19]))
    radius = 0.5 * (d[k] + d[k + 1])
    inside = lam[:k + 1]
    fpm = fk.feastinit()
    r = fk.feast_general(A, B, center, radius, M0=max(2 * len(inside), 24), fpm=fpm, engine=adj, two_sided=True, solver="sparse_direct")
    ts = r.stats["two_sided"]
    print("info %d M %d loops %d epsout %.2e plan %s fell_back %s" % (r.info, r.M, r.loop, r.epsout, ts["direct_plan"], ts["fell_back"]))
    assert r.info == 0 and r.M == len(inside), (r.info, r.M, len(inside))
    assert ts["direct_plan"].startswith("band LU") and ts["fell_back"] is True
    assert ts["adjoint_factorizations"] == 0
    got = np.sort_complex(r.lambda_[:r.M])
    want = np.sort_complex(inside)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    X, Y = r.q[:, :r.M], r.q_left[:, :r.M]
    lam_dev = r.lambda_[:r.M]
    rr = np.linalg.norm(A @ X - (B @ X) * lam_dev, axis=0) / np.linalg.norm(X, axis=0)
    rl = np.linalg.norm(A.conj().T @ Y - (B.conj().T @ Y) * np.conj(lam_dev), axis=0) / np.linalg.norm(Y, axis=0)
    print("host residuals: right %.2e left %.2e" % (rr.max(), rl.max()))
    assert rr.max() <= 1e-10 and rl.max() <= 1e-10
    G = Y.conj().T @ (B @ X)
    assert np.abs(np.diag(G) - 1.0).max() <= 1e-12


# ---- 6. a small zero-diagonal case against the host restatement -----------------------------------------------------------------
_zd = {}


def _zero_diagonal_case():
    """random_zero_diagonal(200, 6, 0.5, 3, False), B = I; the circle by the rule of tests/two_sided_sparse_cases.py (centre 0,
    radius 0.149, 9 eigenvalues, gap ratio 1.85); M0 = 18, 8 nodes: with the default 16 the restatement stalls at 2e-12,
    with 8 it converges (info 0) in 3 loops to 3.9e-13, smallest overlap 0.117."""
    if not _zd:
        A = random_zero_diagonal(200, 6, 0.5, 3, False)
        Ad = A.toarray()
        lam = sla.eigvals(Ad)
        center, radius, k, ratio = sc.choose_circle(lam)
        inside = lam[np.abs(lam - center) < radius]
        fpm = fk.feastinit()
        fpm[3], fpm[4], fpm[8] = 12, 20, 8
        ref = two_sided_reference(Ad, None, center, radius, 2 * k, fpm)
        _zd.update(A=A, center=center, radius=radius, k=k, ratio=ratio, lam_in=inside[np.argsort(np.abs(inside) ** 2)], ref=ref)
    return _zd


@pytest.mark.parametrize("forced", [False, True], ids=["own-plan", "forced-fallback"])
def test_driver_zero_diagonal_against_restatement(adj, own_plan, monkeypatch, forced):
    case = _zero_diagonal_case()
    ref = case["ref"]
    assert (case["center"], case["radius"], case["k"]) == (0j, 0.149, 9) and abs(case["ratio"] - 1.85) < 0.01
    assert ref["info"] == 0 and ref["M"] == 9
    if forced:
        monkeypatch.setenv("FH_MF_MAX_MULTIPLIER", "0")
    fpm = fk.feastinit()
    fpm[3], fpm[4], fpm[8] = 12, 20, 8
    adj._problem_fp = None                   # a fresh plan for either run
    res = fk.feast_general(case["A"], None, case["center"], case["radius"], M0=18, fpm=fpm, engine=adj, two_sided=True,
                           solver="sparse_direct")
    ts = res.stats["two_sided"]
    print("loops %d (restatement %d) epsout %.2e plan %s fell_back %s" % (res.loop, ref["loop"], res.epsout, ts["direct_plan"], ts["fell_back"]))
    assert res.info == 0 and res.M == case["k"]
    if forced:
        assert ts["direct_plan"].startswith("band LU") and ts["fell_back"] is True
    assert ts["adjoint_factorizations"] == 0
    idx = _match(res.lambda_, case["lam_in"])
    assert np.abs(res.lambda_ - case["lam_in"][idx]).max() <= 1e-10
    ridx = _match(res.lambda_, ref["lam"][:ref["M"]])
    overlap = ref["overlap"][ridx]
    print("overlap device", ts["overlap"], "restatement", overlap)
    assert (np.abs(ts["overlap"] - overlap) <= 1e-8 * overlap).all()
    assert res.loop <= ref["loop"] + 2


# ---- 7. the one-sided call is unchanged -----------------------------------------------------------------------------------------
def test_one_sided_call_unchanged_by_forced_fallback(own_plan, monkeypatch):
    case = sc.make_case(*sc.PARAMS[1])
    fpm = fk.feastinit()
    fpm[3], fpm[4] = 12, 20
    kw = dict(M0=case["M0"], fpm=fpm, solver="sparse_direct")
    eng = fk.HipEngine(0)
    try:
        before = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, **kw)
        monkeypatch.setenv("FH_MF_MAX_MULTIPLIER", "0")
        two = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, two_sided=True, **kw)
        monkeypatch.delenv("FH_MF_MAX_MULTIPLIER")
        after = fk.feast_general(case["A"], case["B"], case["center"], case["radius"], engine=eng, **kw)
    finally:
        eng.close()
    assert two.q_left is not None and two.info == 0 and two.stats["two_sided"]["fell_back"] is True
    assert before.q_left is None and after.q_left is None and "two_sided" not in after.stats
    assert before.M == after.M == case["k"] and before.loop == after.loop
    assert np.array_equal(before.lambda_, after.lambda_) and np.array_equal(before.q, after.q) and np.array_equal(before.res, after.res)
