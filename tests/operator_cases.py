"""The inputs of test_gpu_operator.py, shared with test_operator_host.py (which asserts on the references alone the conditions
the device comparison rests on): operator callbacks built from a matrix, a genuinely matrix-free Laplacian, and the sweep
cases.  The truncation cases are those of krylov_cases.py / gmres_cases.py on their dense pencils."""
import functools

import numpy as np
import scipy.sparse as sp

import gmres_cases as gc
import krylov_cases as kc

# ---- callbacks built from a matrix: a torch dense product on the uploaded copy -----------------------------------------------------
def dense_of(M):
    return None if M is None else (M.toarray() if sp.issparse(M) else np.asarray(M))


def matrix_mul(engine, M, real=True):
    """mul(Y, X) for engine.set_operator(..., batched=False): Y = M X with the matrix M resident as a torch tensor.  real: M is
    real and the panels come as their (N, 2 ld) real views; otherwise complex128 (N, ld) panels."""
    torch = engine.torch
    Md = dense_of(M)
    if real:
        assert not np.iscomplexobj(Md)
        T = torch.from_numpy(np.ascontiguousarray(Md, dtype=np.float64)).to(engine.device)
    else:
        T = torch.from_numpy(np.ascontiguousarray(Md, dtype=np.complex128)).to(engine.device)

    def mul(Y, X):
        torch.matmul(T, X, out=Y)
    return mul


def over_nodes(mul):
    """The batched form of a per-node function: one call on (nodes, N, w) tensors."""
    def f(Y, X):
        assert X.dim() == 3 and Y.shape == X.shape
        for e in range(X.shape[0]):
            mul(Y[e], X[e])
    return f


def set_matrix_operator(engine, A, B=None, real=True, symmetric=False, batched=False):
    """The operator handle whose callbacks multiply by the dense A and B."""
    a, b = matrix_mul(engine, A, real), (None if B is None else matrix_mul(engine, B, real))
    if batched:
        a, b = over_nodes(a), (None if b is None else over_nodes(b))
    engine.set_operator(A.shape[0], a, b, real=real, symmetric=symmetric, batched=batched)


# ---- a matrix-free 7-point Laplacian by tensor slicing -------------------------------------------------------------------------------
GRID = (12, 10, 8)


def laplacian_mul(grid=GRID):
    """mul(Y, X) on (N, w) panels, N = nx ny nz in C order: Y = L X for the 7-point Laplacian with Dirichlet ends, formed from
    shifted slices of the panel viewed as (nx, ny, nz, w).  No matrix exists."""
    nx, ny, nz = grid

    def mul(Y, X):
        w = X.shape[-1]
        x, y = X.view(nx, ny, nz, w), Y.view(nx, ny, nz, w)
        y.copy_(x)
        y.mul_(6.0)
        y[1:].sub_(x[:-1]); y[:-1].sub_(x[1:])
        y[:, 1:].sub_(x[:, :-1]); y[:, :-1].sub_(x[:, 1:])
        y[:, :, 1:].sub_(x[:, :, :-1]); y[:, :, :-1].sub_(x[:, :, 1:])
    return mul


def laplacian_eigenvalues(grid=GRID):
    """sum_d 2 - 2 cos(pi k / (n_d + 1)), sorted."""
    one = [2.0 - 2.0 * np.cos(np.pi * np.arange(1, n + 1) / (n + 1)) for n in grid]
    return np.sort((one[0][:, None, None] + one[1][None, :, None] + one[2][None, None, :]).ravel())


def laplacian_matrix(grid=GRID):
    """The same operator as a scipy matrix (host checks only)."""
    T = [sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]) for n in grid]
    I = [sp.identity(n) for n in grid]
    return sp.csr_matrix(sp.kron(sp.kron(T[0], I[1]), I[2]) + sp.kron(sp.kron(I[0], T[1]), I[2]) + sp.kron(sp.kron(I[0], I[1]), T[2]))


def diagonal_b(N):
    """A diagonal B between 1 and 2 (fixed seed)."""
    return 1.0 + np.random.default_rng(7).random(N)


def diagonal_mul(engine, d):
    t = engine.torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).to(engine.device)

    def mul(Y, X):
        engine.torch.mul(X, t[:, None], out=Y)
    return mul


# ---- a small convection-diffusion operator (non-symmetric, real) ---------------------------------------------------------------------
def convection_diffusion(n=(14, 14), beta=(0.4, 0.25)):
    """Upwind-free centred differences of -Laplace u + beta . grad u on an n[0] x n[1] grid, h = 1: N = 196, real, not normal."""
    T = [sp.diags([(-1.0 - 0.5 * b) * np.ones(k - 1), 2.0 * np.ones(k), (-1.0 + 0.5 * b) * np.ones(k - 1)], [-1, 0, 1])
         for k, b in zip(n, beta)]
    I = [sp.identity(k) for k in n]
    return np.asarray((sp.kron(T[0], I[1]) + sp.kron(I[0], T[1])).todense())


# ---- a banded operator for the product at a size where the combine kernel's loop takes more than one trip ----------------------------
def band_mul(engine, N, cplx):
    """mul(Y, X) of the pentadiagonal operator with diagonals d0, d1 (offset 1, both sides) and d3 (offset 3, upper only, so the
    operator is not symmetric), and the same operator on the host in long double: (mul, host)."""
    rng = np.random.default_rng(11)
    d0, d1, d3 = rng.standard_normal(N), rng.standard_normal(N - 1), rng.standard_normal(N - 3)
    if cplx:
        d0 = d0 + 1j * rng.standard_normal(N)
    torch = engine.torch
    t0, t1, t3 = (torch.from_numpy(np.ascontiguousarray(d)).to(engine.device)[:, None] for d in (d0, d1, d3))

    def mul(Y, X):
        torch.mul(X, t0, out=Y)
        Y[:-1].add_(t1 * X[1:]); Y[1:].add_(t1 * X[:-1])
        Y[:-3].add_(t3 * X[3:])

    def host(X):
        ct = np.clongdouble
        X = X.astype(ct)
        Y = d0.astype(ct)[:, None] * X
        Y[:-1] += d1.astype(ct)[:, None] * X[1:]; Y[1:] += d1.astype(ct)[:, None] * X[:-1]
        Y[:-3] += d3.astype(ct)[:, None] * X[3:]
        return Y
    fro = float(np.sqrt((np.abs(d0) ** 2).sum() + 2 * (d1 ** 2).sum() + (d3 ** 2).sum()))
    return mul, host, fro


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
# (module, case name, device solver): the truncation cases the operator handle repeats on the dense pencils
TRUNC = (("kc", "bicgstab-dense-N203-m16", "bicgstab"), ("kc", "cocg-dense-N336-m7", "cocg"), ("gc", "dense-N203-m16-r30", "gmres"))

# (restatement, device solver, rtol, maxit, Ritz warm start) of the Krylov sweeps: 8 nodes, m = 24, the real projection.  From the
# zero guess the nodes need between a few and some tens of steps, so that at maxit = 7 the cap bites; the warm-started sweep adds the shared start residual A q - lambda B q, a product of its own.
SWEEP_M = 24
SWEEPS = (("cocg5", "cocg", 3e-2, 50, False), ("cocg5", "cocg", 3e-2, 7, False), ("cocg5", "cocg", 3e-2, 50, True),
          ("bicgstab", "bicgstab", 3e-2, 50, True), ("bicgstab", "bicgstab", 3e-2, 7, False))
# (BiCGStab from the zero guess at maxit = 50 loses every digit to rounding next to the spectrum -- the drift of the
#  restatement itself is 0.3 there -- so its 50-step sweep is the warm-started one, as in krylov_cases.BICGSTAB_SWEEPS.)
# the GMRES sweep under node batches of 3: the callback sees nodes = 3, 3, 2 on the 8-node contour
GMRES_SWEEP = ("cfg3", 24, True, gc.SWEEP_SETTINGS[1])
GMRES_BATCH = 3


def trunc_case(mod, name, near):
    return (kc if mod == "kc" else gc).trunc_case(name, near)


def sweep_case(method, rtol, maxit, warm):
    return kc.sweep_case(method, rtol, maxit, SWEEP_M, warm)


def gmres_sweep_case():
    return gc.sweep_case(*GMRES_SWEEP, GMRES_BATCH)


@functools.lru_cache(maxsize=None)
def product_inputs(N, m, cplx):
    """(A, B, X): dense N x N matrices (complex when asked) and an N x m complex block, fixed seeds."""
    rng = np.random.default_rng(100 + N + m)
    A, B = rng.standard_normal((N, N)), rng.standard_normal((N, N))
    if cplx:
        A, B = A + 1j * rng.standard_normal((N, N)), B + 1j * rng.standard_normal((N, N))
    X = rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))
    return A, B, np.asfortranarray(X)


@functools.lru_cache(maxsize=None)
def solve_pair(N, m):
    """(A, B, X) for solves: A a small non-symmetric perturbation, B = 4 I plus one, so that z B - A is well conditioned for
    the shifts the tests use; X an N x m complex block."""
    G, H, X = product_inputs(N, m, False)
    return G / 10.0, 4.0 * np.eye(N) + H / 10.0, X
