"""The sparse direct solver on pencils whose fully-summed front blocks are singular or nearly so.

The multifrontal plan (csrc/fh_mf.hpp, fh_dense.hip fh_mf_*) takes a front's pivots from its fully-summed rows only.  On a
bipartite zero-diagonal Hamiltonian at z = i eps, every leaf whose vertex set is unbalanced between the two colours has a
block -K_leaf + i eps I whose last pivot is ~ i eps: tiny but not zero, while the whole matrix has cond ~ 1e4.  Saddle-point
pencils with a zero constraint block give leaf blocks that are exactly singular.  The library checks the boundary
multipliers of every front and refactors such a matrix with the band LU (partial pivoting over the whole band); these tests
hold every solve to SuperLU and to the fp64 residual recomputed here, so that "rc 0 with a large residual" fails."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feastkit_jl_amd as fk
from feastkit_jl_amd import workloads
from test_gpu_multifrontal import grid_pencil
from test_gpu_wband import check_solve

pytestmark = pytest.mark.gpu

MF, BAND = 2, 1                # engine.band_plan()[3]: multifrontal plan, blocked band plan (what a fallback leaves)


# ---- generators ---------------------------------------------------------------------------------------------------------
def _grid_edges(dims):
    idx = np.arange(int(np.prod(dims))).reshape(dims)
    rows, cols = [], []
    for ax in range(len(dims)):
        a = idx[(slice(None),) * ax + (slice(1, None),)]
        b = idx[(slice(None),) * ax + (slice(None, -1),)]
        rows.append(a.ravel()); cols.append(b.ravel())
    return np.concatenate(rows), np.concatenate(cols), idx


def bipartite_hamiltonian(dims, seed, peierls=False):
    """Tight-binding H on a grid: random real hoppings of either sign (|t| in [0.5, 1.5]), zero diagonal; with random
    Peierls phases on the bonds when `peierls`.  The grid has an even number of sites, so the two colour classes have equal
    size and H is nonsingular for generic hoppings."""
    rng = np.random.default_rng(seed)
    r, c, _ = _grid_edges(dims)
    n = int(np.prod(dims))
    assert n % 2 == 0
    t = rng.uniform(0.5, 1.5, len(r)) * rng.choice([-1.0, 1.0], len(r))
    if peierls:
        t = t * np.exp(2j * np.pi * rng.random(len(r)))
    H = sp.coo_matrix((t, (r, c)), shape=(n, n)).tocsr()
    return (H + H.conj().T).tocsr()


def oseen_pencil(nx, ny, seed, nu=1.0, conv=0.6):
    """[[nu L + C, G^T], [G, 0]] with B = diag(I_v, 0): one velocity unknown per grid node (5-point Laplacian, upwind
    convection), one pressure per grid cell coupled to the cell's four corner velocities with random weights (G has full row
    rank: (nx - 1)(ny - 1) pressures against nx ny velocities, the nx + ny - 1 finite eigenvalues live on ker G)."""
    rng = np.random.default_rng(seed)
    nv = nx * ny
    idx = np.arange(nv).reshape(nx, ny)
    L = sp.diags([4.0 * np.ones(nv)], [0]).tolil()
    for a, b in ((idx[1:], idx[:-1]), (idx[:, 1:], idx[:, :-1])):
        L[a.ravel(), b.ravel()] = -1.0
        L[b.ravel(), a.ravel()] = -1.0
    Cv = sp.lil_matrix((nv, nv))
    Cv[idx[1:].ravel(), idx[1:].ravel()] = conv           # upwind in x: conv (u_i - u_{i-1})
    Cv[idx[1:].ravel(), idx[:-1].ravel()] = -conv
    K = (nu * L.tocsr() + Cv.tocsr()).tocsr()
    cells = np.arange((nx - 1) * (ny - 1)).reshape(nx - 1, ny - 1)
    rows, cols = [], []
    for di in (0, 1):
        for dj in (0, 1):
            rows.append(cells.ravel()); cols.append(idx[di:nx - 1 + di, dj:ny - 1 + dj].ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    G = sp.coo_matrix((rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cols)),
                      shape=(cells.size, nv)).tocsr()
    A = sp.bmat([[K, G.T], [G, None]], format="csr")
    B = sp.diags(np.r_[np.ones(nv), np.zeros(cells.size)]).tocsr()
    return A, B


def convection_zero_diagonal(nx, ny, conv=0.2):
    """-(off-diagonal part of a 2-D upwind convection-diffusion stencil): unsymmetric, zero diagonal, bipartite pattern"""
    r, c, _ = _grid_edges((nx, ny))
    n = nx * ny
    up = np.full(len(r), -1.0 - conv)                       # the upwind neighbour carries the convection
    down = np.full(len(r), -1.0)
    A = sp.coo_matrix((np.r_[up, down], (np.r_[r, c], np.r_[c, r])), shape=(n, n)).tocsr()
    return (-A).tocsr()


def random_zero_diagonal(n, band, density, seed, cplx):
    """Random sparse band matrix (no dominance) whose diagonal is exactly zero."""
    rng = np.random.default_rng(seed)
    nnz = int(density * n * (2 * band + 1))
    i = rng.integers(0, n, nnz)
    j = np.clip(i + rng.integers(-band, band + 1, nnz), 0, n - 1)
    v = rng.standard_normal(nnz) + (1j * rng.standard_normal(nnz) if cplx else 0.0)
    A = sp.coo_matrix((v, (i, j)), shape=(n, n)).tocsr()
    A = (A + 0.7 * A.T).tolil()                               # symmetric pattern, unsymmetric values
    A.setdiag(0.0)
    A = A.tocsr()
    A.eliminate_zeros()
    return A


# ---- the bar ------------------------------------------------------------------------------------------------------------
def load(engine, A, B):
    """set the problem and make a fresh plan even when the engine already holds these matrices (a fallback is per plan)"""
    engine._problem_fp = None
    engine.set_problem(A, B)


def cond1(lu, n):
    """1-norm condition estimate of the factored matrix (Hager / Higham through SuperLU's solves)"""
    inv = spla.LinearOperator((n, n), matvec=lambda x: lu.solve(np.asarray(x, complex).ravel()),
                              rmatvec=lambda x: lu.solve(np.asarray(x, complex).ravel(), trans="H"), dtype=complex)
    return spla.onenormest(inv)


def strict_solve(engine, A, B, z, m, seed=5, ref=None):
    """shifted solve on the GPU against SuperLU: rc 0, residual <= max(1e-12, 50 x SuperLU's), and an elementwise error
    relative to max|ref| under 1e-13 cond_1 (1e-9 at cond 1e4) -- a wrong answer with rc 0 fails here"""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
    S = (z * (B if B is not None else sp.identity(n)) - A).tocsc().astype(complex)
    if ref is None:
        lu = spla.splu(S)
        ref = (lu, cond1(lu, n) * spla.onenormest(S))
    lu, cond = ref
    want = lu.solve(X)
    dY, rc = engine.shifted_solve(z, engine.upload(X), m)
    Y = engine.download(dY, m)
    res = np.linalg.norm(S @ Y - X) / np.linalg.norm(X)
    res_ref = np.linalg.norm(S @ want - X) / np.linalg.norm(X)
    err = np.abs(Y - want).max() / np.abs(want).max()
    msg = f"z={z} rc={rc} residual {res:.2e} (SuperLU {res_ref:.2e}) error {err:.2e} cond {cond:.1e}"
    assert rc == 0, msg
    assert res <= max(1e-12, 50 * res_ref), msg
    assert err <= max(1e-12, 1e-13 * cond), msg
    return ref


def strict_solve_all(engine, A, B, z, m, leaves=("8", "24", "64"), precisions=(64, 32), monkeypatch=None):
    """strict_solve under every leaf size and factor precision on fresh plans; returns the plan kinds after each solve"""
    plans = []
    ref = None
    for leaf in leaves:
        monkeypatch.setenv("FH_MF_LEAF", leaf)
        for prec in precisions:
            load(engine, A, B)
            engine.set_solver("banded", rtol=1e-13, factor_precision=prec)
            assert engine.band_plan()[3] == MF
            ref = strict_solve(engine, A, B, z, m, seed=int(leaf) + prec, ref=ref)
            plans.append(engine.band_plan()[3])
    return plans


@pytest.fixture
def force_mf(monkeypatch):
    monkeypatch.setenv("FH_MF", "1")
    monkeypatch.delenv("FH_WBAND", raising=False)


@pytest.fixture
def own_plan(monkeypatch):
    for v in ("FH_MF", "FH_MF_LEAF", "FH_WBAND"):
        monkeypatch.delenv(v, raising=False)


# ---- shifted solves on forced multifrontal plans --------------------------------------------------------------------------
BIPARTITE = {
    "grid2d": lambda: (bipartite_hamiltonian((40, 50), 11), None),
    "grid3d": lambda: (bipartite_hamiltonian((12, 12, 14), 12), None),
    "peierls2d": lambda: (bipartite_hamiltonian((40, 50), 13, peierls=True), None),
    "grid2d_mildB": lambda: (bipartite_hamiltonian((40, 50), 14),
                             sp.diags(1.0 + 0.2 * np.random.default_rng(15).random(2000)).tocsr()),
}


@pytest.mark.parametrize("eps", [1e-3, 1e-7, 1e-11])
@pytest.mark.parametrize("family", sorted(BIPARTITE))
def test_bipartite_hamiltonian_at_i_eps(engine, force_mf, monkeypatch, family, eps):
    A, B = BIPARTITE[family]()
    plans = strict_solve_all(engine, A, B, 1j * eps, 12, monkeypatch=monkeypatch)
    if eps <= 1e-7:                     # a pass must not be luck: the rejected pivots were seen and the band LU took over
        assert all(p == BAND for p in plans), plans


SHIFTS = [0.0, 0.4 + 0.3j, -0.7 + 0.05j, 1e-4 + 1e-6j]


@pytest.mark.parametrize("z", SHIFTS)
def test_oseen_saddle_point(engine, force_mf, monkeypatch, z):
    A, B = oseen_pencil(24, 24, 3)
    strict_solve_all(engine, A, B, z, 12, monkeypatch=monkeypatch)


@pytest.mark.parametrize("z", SHIFTS)
def test_convection_zero_diagonal(engine, force_mf, monkeypatch, z):
    A = convection_zero_diagonal(36, 40)
    strict_solve_all(engine, A, None, z, 12, monkeypatch=monkeypatch)


@pytest.mark.parametrize("z", [0.0, 0.3 + 0.2j, 1e-5j])
@pytest.mark.parametrize("cplx", [False, True])
def test_random_zero_diagonal(engine, force_mf, monkeypatch, cplx, z):
    A = random_zero_diagonal(1500, 30, 0.1, 21 + cplx, cplx)
    strict_solve_all(engine, A, None, z, 12, leaves=("8", "64"), monkeypatch=monkeypatch)


# ---- the library's own plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peierls", [False, True])
def test_own_plan_bipartite(engine, own_plan, peierls):
    A = bipartite_hamiltonian((16, 16, 16), 31 + peierls, peierls=peierls)
    load(engine, A, None)
    engine.set_solver("banded")
    assert engine.band_plan()[3] == MF
    strict_solve(engine, A, None, 1e-9j, 16)
    assert engine.band_plan()[3] == BAND
    # the band plan stays for this matrix: a second shift is factored and solved there
    strict_solve(engine, A, None, 0.01 + 1e-3j, 16, seed=8)
    assert engine.band_plan()[3] == BAND


# ---- contour_apply across a fallback ------------------------------------------------------------------------------------------
def test_contour_apply_across_fallback(engine, force_mf):
    A = bipartite_hamiltonian((40, 50), 41)
    n = A.shape[0]
    load(engine, A, None)
    engine.set_solver("banded")
    assert engine.band_plan()[3] == MF
    Z = np.linspace(-0.02, 0.02, 8) + 1e-9j
    W = np.exp(1j * np.arange(8)) / 8
    engine.set_contour(Z, W, 2.0)
    engine.set_real_projection(False)
    Q = fk.seeded_subspace(n, 24)
    dP, status, st = engine.contour_apply(engine.upload(Q), 24)
    assert np.all(status[:8] == 0), status
    assert st["factorizations"] >= 8
    assert engine.band_plan()[3] == BAND
    I = sp.identity(n, format="csc")
    want = sum(2 * W[e] * spla.splu((Z[e] * I - A).tocsc().astype(complex)).solve(Q.astype(complex)) for e in range(8))
    got = engine.download(dP, 24)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    dP2, status, st2 = engine.contour_apply(engine.upload(Q), 24)
    assert st2["factorizations"] == 0 and np.all(status[:8] == 0)
    assert np.array_equal(engine.download(dP2, 24), got)


# ---- benign pencils keep the multifrontal plan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cplx,unsym", [((12, 10, 8), True, False), ((20, 16, 9), False, True), ((25, 20, 12), True, True)])
def test_benign_grid_pencils_keep_the_plan(engine, force_mf, shape, cplx, unsym):
    A, B = grid_pencil(*shape, seed=sum(shape), cplx=cplx, unsym=unsym)
    load(engine, A, B)
    engine.set_solver("banded")
    assert engine.band_plan()[3] == MF
    # (test_gpu_multifrontal.py's shifts and bar: these random pencils without diagonal dominance have boundary multipliers
    # up to ~300 there, residuals up to ~60 x SuperLU's -- inside the bound, so they must stay on the multifrontal plan)
    for k, z in enumerate((0.3 + 0.8j, -0.4 + 0.3j)):
        check_solve(engine, A, B, z, 8, seed=k)
    assert engine.band_plan()[3] == MF
    load(engine, A, None)
    engine.set_solver("banded")
    assert engine.band_plan()[3] == MF
    check_solve(engine, A, None, -0.2 + 0.05j, 8)
    assert engine.band_plan()[3] == MF


@pytest.mark.parametrize("dims,interval", [((30, 20, 12), (0.0, 0.25)), ((30, 20, 13), (0.0, 0.25))])
def test_benign_laplacian_contours_keep_the_plan(engine, own_plan, monkeypatch, dims, interval):
    """the reduced cfg 3 Laplacian (forced plan) and the cfg 3 family at 7800 unknowns (own plan) on the bench contour
    (16 Gauss nodes, fpm[18] = 4000) and on the default one: every node factored on the multifrontal plan, no fallback"""
    if dims == (30, 20, 12):
        monkeypatch.setenv("FH_MF", "1")
    A, B, _ = workloads.laplacian_3d_pencil(*dims)
    n = A.shape[0]
    load(engine, A, B)
    engine.set_solver("banded")
    assert engine.band_plan()[3] == MF
    Q = fk.seeded_subspace(n, 16)
    for ne, aspect in ((16, 4000), (8, 100)):
        fpm = fk.feastdefault(fk.feastinit())
        fpm[2], fpm[16], fpm[18] = ne, 0, aspect
        Z, W = fk.feast_contour(*interval, fpm)
        engine.set_contour(Z, W, 2.0)
        engine.set_real_projection(False)
        dP, status, st = engine.contour_apply(engine.upload(Q), 16)
        assert np.all(status[:ne] == 0) and st["factorizations"] == ne
        assert engine.band_plan()[3] == MF
        if aspect == 4000:
            z_bench = Z[0]
    # the bench contour's node nearest the real axis against SuperLU
    strict_solve(engine, A, B, z_bench, 8)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _finite_eigs_near(A, B, sigma, k):
    """the k finite eigenvalues of A x = lambda B x nearest sigma (shift-invert Arnoldi with SuperLU; B may be singular)"""
    n = A.shape[0]
    lu = spla.splu((A - sigma * B).tocsc().astype(complex))
    op = spla.LinearOperator((n, n), matvec=lambda x: lu.solve((B @ x).astype(complex)), dtype=complex)
    mu = spla.eigs(op, k=k, which="LM", tol=1e-14, return_eigenvectors=False, v0=np.ones(n, complex))
    lam = sigma + 1.0 / mu
    return lam[np.argsort(np.abs(lam - sigma))]


def test_feast_general_saddle_point(engine, own_plan, monkeypatch):
    """the default call on a saddle-point pencil, unknowns numbered node by node (each velocity followed by the pressure of
    its cell: a band of ~2 ny, so the driver's choice is the sparse direct solver, not the dense LU of the expanded matrix).
    Its multifrontal plan (forced: the library's own choice for this 2-D pencil is the band) meets exactly singular leaf
    blocks and hands the matrix over to the band LU inside the driver's first sweep."""
    monkeypatch.setenv("FH_MF", "1")
    nx = ny = 45
    A, B = oseen_pencil(nx, ny, 17)                  # N = 3961, 89 finite eigenvalues
    order = []
    for i in range(nx):
        for j in range(ny):
            order.append(i * ny + j)
            if i < nx - 1 and j < ny - 1:
                order.append(nx * ny + i * (ny - 1) + j)
    order = np.asarray(order)
    A, B = A[order][:, order].tocsr(), B[order][:, order].tocsr()
    load(engine, A, B)
    assert engine.band_plan()[3] == MF
    center = 2.0 + 0.0j
    lam = _finite_eigs_near(A, B, center, 30)
    d = np.abs(lam - center)
    k = 8 + int(np.argmax(d[9:20] - d[8:19]))         # the widest gap between the 9th and the 20th nearest
    radius = 0.5 * (d[k] + d[k + 1])
    inside = lam[:k + 1]
    fpm = fk.feastinit()
    r = fk.feast_general(A, B, center, radius, M0=max(2 * len(inside), 24), fpm=fpm, engine=engine)
    assert engine.band_plan()[3] == BAND           # only the sparse direct solver's fallback changes the plan
    assert r.info == 0 and r.M == len(inside), (r.info, r.M, len(inside))
    got = np.sort_complex(r.lambda_[:r.M])
    want = np.sort_complex(inside)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    X = r.q[:, :r.M]
    res = np.linalg.norm(A @ X - (B @ X) * r.lambda_[:r.M], axis=0) / np.linalg.norm(X, axis=0)
    assert res.max() <= 1e-10, res.max()


@pytest.mark.parametrize("aspect", [None, 10])
def test_feast_bipartite_interior_window(engine, own_plan, aspect):
    """the default call on a tight-binding H (N = 3840; the library's own plan is the multifrontal one) with an interior
    window around E = 0, on the default circle and on a flat ellipse (fpm[18] = 10) whose nodes come within 5e-4 of the
    origin: there the rejected pivots hand the matrix to the band LU in the middle of the driver's first sweep.
    (M0 = 16 for 6 eigenvalues: with the window's neighbours at 1.2 - 1.7 delta the 8-node filter needs the room; the
    reference algorithm with SuperLU solves stops with info 5 on a spurious Ritz value at M0 = 1.5 M on wider windows of
    this H as well.)"""
    H = bipartite_hamiltonian((16, 16, 15), 51)
    lam_all = np.linalg.eigvalsh(H.toarray())
    a = np.unique(np.round(np.abs(lam_all), 12))
    delta = float(np.sqrt(a[2] * a[3]))              # the 3rd and 4th distinct |lambda|: 3.8e-3 and 5.5e-3
    inside = lam_all[np.abs(lam_all) < delta]
    assert len(inside) == 6
    load(engine, H, None)
    assert engine.band_plan()[3] == MF
    fpm = fk.feastinit()
    if aspect is not None:
        fpm[18] = aspect
    r = fk.feast(H, None, (-delta, delta), M0=16, fpm=fpm, engine=engine)
    if aspect is not None:
        assert engine.band_plan()[3] == BAND
    assert r.info == 0 and r.M == len(inside), (r.info, r.M, len(inside))
    assert np.abs(np.sort(r.lambda_[:r.M]) - np.sort(inside)).max() <= 1e-10
    X = r.q[:, :r.M]
    res = np.linalg.norm(H @ X - X * r.lambda_[:r.M], axis=0) / np.linalg.norm(X, axis=0)
    assert res.max() <= 1e-10, res.max()
