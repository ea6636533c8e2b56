"""Host restatement (numpy only) of the blocked band LU of csrc/fh_dense.hip (fh_wband_factor) and of its two substitutions,
fh_wband_solve and fh_wband_solve_adjoint, in the block order the device runs them.

The factorisation is ZGBTRF's: partial pivoting over the rows a block column reaches, and the interchanges of block column
b are applied inside that block column and to its right, NOT to the block columns left of it.  With P_b the interchanges of
block b and L_b the identity plus the block column's multipliers,

    S = P_0 L_0 P_1 L_1 ... P_last L_last U,

so the forward solve applies, for b ascending, the interchanges of b, L11^-1 and the update of the rows below, and then U^-1
block by block descending; the adjoint solve S^H y = x reads the product from the other end:

    up     U^H w = x, blocks ascending: w_b = U11^-H x_b, then x[i] -= sum_k conj(U[K0+k, i]) w[K0+k] for the rows i below the
           block as far as the block row of U reaches, [Kend, Kend + kl + ku)                        (right-looking)
    down   blocks descending: v_b -= L21^H v[Kend:nr), v_b = L11^-H v_b, then the interchanges of b in REVERSE order on the
           rows [K0, nr), nr = min(N, Kend + kl)                                                    (left-looking)

The down sweep cannot push its update into the earlier blocks ahead of time: the interchanges of block b move rows of
[Kend, nr) that those blocks have yet to read.  `nb` is the block width (128 on the device; the tests use 4 and 8).  Every
slice below is the range the device kernels are launched on, so the restatement pins the ranges as well as the order."""
import numpy as np
import scipy.linalg as sla


def band_lu_blocked(S, kl, ku, nb):
    """-> (LU, piv): multipliers below the diagonal, U on and above it, piv[j] the global row exchanged with row j."""
    N = S.shape[0]
    A = np.array(S, dtype=complex)
    piv = np.arange(N)
    for K0 in range(0, N, nb):
        Kend = min(N, K0 + nb)
        nr = min(N, Kend + kl)                # rows the block column reaches
        nc = min(N, Kend + kl + ku)           # columns its pivot rows reach
        for j in range(K0, Kend):
            p = j + int(np.argmax(np.abs(A[j:nr, j])))
            piv[j] = p
            if p != j:
                A[[j, p], K0:Kend] = A[[p, j], K0:Kend]          # inside the block column only
            A[j + 1:nr, j] /= A[j, j]
            A[j + 1:nr, j + 1:Kend] -= np.outer(A[j + 1:nr, j], A[j, j + 1:Kend])
        if Kend >= N:
            break
        for j in range(K0, Kend):                                # to the right only
            p = piv[j]
            if p != j:
                A[[j, p], Kend:nc] = A[[p, j], Kend:nc]
        L11 = np.tril(A[K0:Kend, K0:Kend], -1) + np.eye(Kend - K0)
        A[K0:Kend, Kend:nc] = sla.solve_triangular(L11, A[K0:Kend, Kend:nc], lower=True, unit_diagonal=True)
        A[Kend:nr, Kend:nc] -= A[Kend:nr, K0:Kend] @ A[K0:Kend, Kend:nc]
    return A, piv


def _blocks(N, nb):
    return [(K0, min(N, K0 + nb)) for K0 in range(0, N, nb)]


def _L11(LU, K0, Kend):
    return np.tril(LU[K0:Kend, K0:Kend], -1) + np.eye(Kend - K0)


def _U11(LU, K0, Kend):
    return np.triu(LU[K0:Kend, K0:Kend])


def solve_forward(LU, piv, kl, ku, nb, X):
    """S y = x in the order of wband_solve_launch"""
    N = LU.shape[0]
    Y = np.array(X, dtype=complex)
    for K0, Kend in _blocks(N, nb):
        nr = min(N, Kend + kl)
        for j in range(K0, Kend):
            p = piv[j]
            if p != j:
                Y[[j, p]] = Y[[p, j]]
        Y[K0:Kend] = sla.solve_triangular(_L11(LU, K0, Kend), Y[K0:Kend], lower=True, unit_diagonal=True)
        Y[Kend:nr] -= LU[Kend:nr, K0:Kend] @ Y[K0:Kend]
    for K0, Kend in reversed(_blocks(N, nb)):
        Y[K0:Kend] = sla.solve_triangular(_U11(LU, K0, Kend), Y[K0:Kend], lower=False)
        r0 = max(0, K0 - kl - ku)
        Y[r0:K0] -= LU[r0:K0, K0:Kend] @ Y[K0:Kend]
    return Y


def solve_adjoint(LU, piv, kl, ku, nb, X, reverse_swaps=True):
    """S^H y = x in the order of wband_solve_adjoint_launch.  reverse_swaps=False applies each block's interchanges first to
    last, as the forward sweep does: the wrong inverse whenever two interchanges of a block share a row (tests)."""
    N = LU.shape[0]
    Y = np.array(X, dtype=complex)
    for K0, Kend in _blocks(N, nb):                              # up: U^H w = x
        Y[K0:Kend] = sla.solve_triangular(_U11(LU, K0, Kend).conj().T, Y[K0:Kend], lower=True)
        r1 = min(N, Kend + kl + ku)
        Y[Kend:r1] -= LU[K0:Kend, Kend:r1].conj().T @ Y[K0:Kend]
    for K0, Kend in reversed(_blocks(N, nb)):                    # down: L_b^H, then the interchanges of b undone
        nr = min(N, Kend + kl)
        Y[K0:Kend] -= LU[Kend:nr, K0:Kend].conj().T @ Y[Kend:nr]
        Y[K0:Kend] = sla.solve_triangular(_L11(LU, K0, Kend).conj().T, Y[K0:Kend], lower=False, unit_diagonal=True)
        order = range(Kend - 1, K0 - 1, -1) if reverse_swaps else range(K0, Kend)
        for j in order:
            p = piv[j]
            if p != j:
                Y[[j, p]] = Y[[p, j]]
    return Y


def random_band(N, kl, ku, seed, zero_every=1):
    """Random unsymmetric complex band matrix without dominance; the diagonal entries i with (i + 1) % zero_every == 0 are exactly
    zero, which forces an interchange in those columns (zero_every = 2 for a tridiagonal matrix of odd order: with the whole
    diagonal zero it would be singular)."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    i, j = np.indices((N, N))
    S[(i - j > kl) | (j - i > ku)] = 0.0
    d = np.arange(zero_every - 1, N, zero_every)
    S[d, d] = 0.0
    return S
