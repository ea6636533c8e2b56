"""Sparse matrix polynomials for the tests of feast_polynomial(..., solver="sparse_direct").

* mixed_pattern_coeffs: coefficients whose patterns differ (a stencil, random local couplings, a coefficient without any
  entry, rows that are empty in one coefficient), real or mixed real / complex -- for the union-pattern ingest and the device
  primitives.  P(lambda) = L + (4 - lambda) I + small couplings: diagonally dominant on the circle of the solve and product
  tests (|z| <= 0.85), and with eigenvalues near those of L + 4 I, a few of which sweep_circle encloses (a contour sum with
  nothing inside is zero up to the quadrature error, and no relative error can be read off it).
* damped_case: K + lambda C + lambda^2 M on a 2-D grid with the spectrum known in closed form, and its "scaled" variant.
* saddle_quadratic: a quadratic whose coefficients all have a structurally zero diagonal block (the fallback)."""
import functools

import numpy as np
import scipy.sparse as sp

NE = 16
FPM3 = 10
CENTER = 0.2 + 0.1j          # contour of the primitive tests
RADIUS = 0.6

# primitive shapes: grid (nx, ny, nz) -> N = 63, 286, 320, none a multiple of 64
GRIDS = [(9, 7, 1), (13, 11, 2), (20, 16, 1)]


def laplacian(nx, ny, nz=1):
    """Dirichlet 5-point (nz = 1) / 7-point Laplacian, CSR, x fastest (grid index i + nx (j + ny k)) like workloads.laplacian_3d_pencil."""
    def t(n):
        return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr") if n > 1 else sp.csr_matrix((1, 1))
    I = [sp.identity(n, format="csr") for n in (nx, ny, nz)]
    L = sp.kron(I[2], sp.kron(I[1], t(nx))) + sp.kron(I[2], sp.kron(t(ny), I[0])) + sp.kron(t(nz), sp.kron(I[1], I[0]))
    L = sp.csr_matrix(L)
    L.eliminate_zeros()
    return L


def _local_random(N, reach, per_row, rng, cplx):
    """per_row entries per row at random columns within `reach` of the diagonal, values in [-1, 1] (x (1 + i) range if cplx)"""
    rows = np.repeat(np.arange(N), per_row)
    cols = np.clip(rows + rng.integers(-reach, reach + 1, len(rows)), 0, N - 1)
    vals = rng.uniform(-1, 1, len(rows)) + (1j * rng.uniform(-1, 1, len(rows)) if cplx else 0.0)
    return sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr()


@functools.lru_cache(maxsize=None)
def mixed_pattern_coeffs(grid, d, cplx, seed=20260701):
    """-> tuple of d + 1 CSR coefficients (shared: not to be modified).  A_0 = L + 4 I; A_1 = -I + 0.025 R_1 with every
    fifth row empty; A_k = 0.2 x 8^-k R_k above (small against A_0 up to |lambda| = 8), R_k random local couplings, complex for
    odd k when cplx (the even ones stay real: mixed input); for d >= 3, A_2 has no entry at all."""
    nx, ny, nz = grid
    N = nx * ny * nz
    rng = np.random.default_rng([seed, N, d, int(cplx)])
    out = [sp.csr_matrix(laplacian(nx, ny, nz) + 4.0 * sp.identity(N))]
    for k in range(1, d + 1):
        if d >= 3 and k == 2:
            out.append(sp.csr_matrix((N, N)))
            continue
        R = 0.2 * 8.0 ** -k * _local_random(N, nx * ny + 1 if nz > 1 else nx + 1, 3, rng, cplx and k % 2 == 1)
        if k == 1:
            R = R - sp.identity(N)
        R = R.tolil()
        if k == 1:
            for i in range(3, N, 5):
                R[i, :] = 0.0
        R = R.tocsr()
        R.eliminate_zeros()
        out.append(R)
    return tuple(out)


def sweep_circle(grid):
    """A circle with eigenvalues of mixed_pattern_coeffs(grid, ...) inside.  They lie within about 0.2 of the eigenvalues
    4 + mu of L + 4 I (the couplings are that small up to |lambda| = 8), so: centre 4.3, near the low end, and the radius in the
    middle of the widest gap among the 4th .. 10th nearest of the 4 + mu -> (centre, radius)."""
    mu = 4.0
    for n in grid:
        if n > 1:
            mu = np.add.outer(mu, 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1)))
    dist = np.sort(np.abs(np.ravel(mu) - 4.3))
    j = 3 + int(np.argmax(dist[4:10] - dist[3:9]))               # the circle holds dist[0 .. j]
    return 4.3 + 0.0j, float(0.5 * (dist[j] + dist[j + 1]))


def dense(coeffs):
    return [np.asarray(c.toarray()) for c in coeffs]


def random_block(rows, cols, seed):
    rng = np.random.default_rng([seed, rows, cols])
    return np.asfortranarray(rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols)))


# ---- the analytic construction ---------------------------------------------------------------------------------------------
# (nx, ny, center, radius, k inside, M0, loops of the restatement)
DAMPED = {"20x16": (20, 16, -0.055 + 0.36j, 0.16, 5, 4, 4), "24x18": (24, 18, -0.053 + 0.30j, 0.14, 5, 3, 5)}
# driver cases of the device test: (grid, scaled)
DRIVER_CASES = [("20x16", False), ("24x18", True)]
DRIVER_IDS = ["20x16-monic-real", "24x18-scaled-complex"]


@functools.lru_cache(maxsize=None)
def damped_case(name, scaled):
    """A_0 = L, A_1 = 0.1 I + 0.05 L, A_2 = I on the nx x ny grid: the eigenvalues are the roots of
    lambda^2 + (0.1 + 0.05 mu_pq) lambda + mu_pq = 0, mu_pq = 4 - 2 cos(p pi / (nx + 1)) - 2 cos(q pi / (ny + 1)).
    scaled: every coefficient times one complex diagonal D = diag(1 + 0.5 u + 0.3 i v), u, v uniform in [-1, 1]: same spectrum,
    non-monic, complex.  -> dict(coeffs (CSR), N, center, radius, k, M0, loop, lam_in)."""
    nx, ny, center, radius, k, M0, loop = DAMPED[name]
    N = nx * ny
    L = laplacian(nx, ny)
    I = sp.identity(N, format="csr")
    coeffs = [L, sp.csr_matrix(0.1 * I + 0.05 * L), I]
    if scaled:
        rng = np.random.default_rng([20260702, nx, ny])
        D = sp.diags(1.0 + 0.5 * rng.uniform(-1, 1, N) + 0.3j * rng.uniform(-1, 1, N))
        coeffs = [sp.csr_matrix(D @ c) for c in coeffs]
    mu = (4.0 - 2.0 * np.cos(np.arange(1, nx + 1) * np.pi / (nx + 1))[None, :] - 2.0 * np.cos(np.arange(1, ny + 1) * np.pi / (ny + 1))[:, None]).ravel()
    b = 0.1 + 0.05 * mu
    root = np.sqrt((b * b - 4.0 * mu).astype(complex))
    lam = np.concatenate([(-b + root) / 2.0, (-b - root) / 2.0])
    lam_in = lam[np.abs(lam - center) <= radius]
    return {"coeffs": tuple(coeffs), "N": N, "center": center, "radius": radius, "k": k, "M0": M0, "loop": loop,
            "lam_in": np.sort_complex(lam_in), "lam_all": lam}


# ---- the fallback ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def saddle_quadratic(nx=12, ny=10, seed=3):
    """P(lambda) = [[K + lambda C + lambda^2 I, G^T], [G, 0]]: one velocity per grid node (K the 5-point Laplacian, C = 0.1 I +
    0.05 K), one pressure per grid cell coupled to its four corner velocities with random weights.  The pressure block of
    EVERY coefficient is structurally zero, so a front whose fully-summed block holds a pressure without its velocities has
    an exactly zero pivot row for every z.  Unknowns numbered node by node.  2 (nx + ny - 1) finite eigenvalues (on ker G).
    -> dict(coeffs (CSR), N, center, radius, lam_in): the circle holds the eigenvalues of smallest positive imaginary part up
    to the widest gap among the 3rd .. 7th."""
    import scipy.linalg as sla
    rng = np.random.default_rng(seed)
    nv = nx * ny
    idx = np.arange(nv).reshape(nx, ny)
    K = laplacian(nx, ny)
    cells = np.arange((nx - 1) * (ny - 1)).reshape(nx - 1, ny - 1)
    rows, cols = [], []
    for di in (0, 1):
        for dj in (0, 1):
            rows.append(cells.ravel())
            cols.append(idx[di:nx - 1 + di, dj:ny - 1 + dj].ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    G = sp.coo_matrix((rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows)), (rows, cols)), shape=(cells.size, nv)).tocsr()
    Iv = sp.identity(nv, format="csr")
    A0 = sp.bmat([[K, G.T], [G, None]], format="csr")
    A1 = sp.bmat([[0.1 * Iv + 0.05 * K, None], [None, sp.csr_matrix((cells.size, cells.size))]], format="csr")
    A2 = sp.bmat([[Iv, None], [None, sp.csr_matrix((cells.size, cells.size))]], format="csr")
    order = []
    for i in range(nx):
        for j in range(ny):
            order.append(i * ny + j)
            if i < nx - 1 and j < ny - 1:
                order.append(nv + i * (ny - 1) + j)
    order = np.asarray(order)
    coeffs = [sp.csr_matrix(A[order][:, order]) for A in (A0, A1, A2)]
    N = nv + cells.size
    # the finite spectrum from the explicit companion (N of a few hundred)
    Z, I = np.zeros((N, N)), np.eye(N)
    d0, d1, d2 = (c.toarray() for c in coeffs)
    lam = sla.eigvals(np.block([[Z, I], [-d0, -d1]]), np.block([[I, Z], [Z, d2]]))
    lam = lam[np.isfinite(lam) & (np.abs(lam) < 1e6)]
    up = lam[lam.imag > 1e-8]
    up = up[np.argsort(up.imag)]
    first = up[:8]
    center = complex(np.mean(first[:3]))
    dist = np.sort(np.abs(up - center))
    j = 2 + int(np.argmax(dist[3:8] - dist[2:7]))            # the circle holds dist[0 .. j]
    radius = 0.5 * (dist[j] + dist[j + 1])
    lam_in = lam[np.abs(lam - center) <= radius]
    return {"coeffs": tuple(coeffs), "N": N, "center": center, "radius": float(radius), "lam_in": np.sort_complex(lam_in),
            "gap": float((dist[j + 1] - dist[j]) / radius)}
