"""Sparse pencils with ragged rows, for the CSR product and Krylov kernels (fh_sparse.hip) and their ingest (fh_ingest.hpp).

The other generators of the suite give rows of one kind: the 7-point stencil (at most 7 entries, full diagonal, sizes that
are multiples of 8) and uniform random couplings around a full diagonal (about 13 entries).  ragged_pair builds the
pattern on purpose instead; with S = the union pattern of A and B (what the device stores):

  ladder     one row of S with exactly L entries for every L of LADDER that fits (ladder_lengths(N)): 1 .. 9 around the
             chunk of 8 of k_spmm_row, 15 .. 17 and 31 .. 33 around the 16 nonzeros k_spmm loads per trip, 24 / 25 and
             64 / 65 around three and eight chunks.  The row with one entry (LONER) holds its diagonal alone; the row with
             two its diagonal and the hub: their largest column is the diagonal (no swap at ingest).
  hub        row and column HUB = 3 couple to every other row but the loner (and the isolated ones), weakly (<= 0.01):
             N - 1 entries (fewer by the isolated rows).  Its block of a renumbered matrix has far more than 160 outside
             rows, and N = 1003 is renumbered at ingest by default (N >= 512, kl + ku > 512) while N = 331 is not.
  last       row and column N - 1 couple to every 5th free row: rows whose largest column is N - 1.
  no diag    A has no diagonal entry on the rows i % 11 == 7; those rows couple to the left only, so with B = I some rows
             have neither a diagonal nor anything right of it.  The other diagonal entries of A are i + 1.
  isolated   b_identity=True: the rows and columns i % 37 == 11 of A are empty (a row of z I - A that is z alone).
  B          symmetric, strictly diagonally dominant, on a pattern of its own: on every ladder row a quarter of the
             couplings is in B only (A holds a zero there on the union pattern), a quarter in both, the rest in A only;
             among the free rows B has random couplings of its own.

Values: real symmetric by default; cplx adds i (T - T^T) with T on half of A's strictly upper entries (Hermitian, same
pattern); unsymmetric scales the strictly lower part entry by entry and adds one-sided couplings among the free rows (an
unsymmetric pattern; the ladder rows keep their lengths).  integer_pair puts small integers on the same patterns and
integer_block is a block of Gaussian integers: every product of the two is exact in binary64 in any order of summation.
numpy / scipy only: the host tests import this module."""
import numpy as np
import scipy.sparse as sp

LADDER = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 64, 65)
HUB = 3
NO_DIAG = (11, 7)          # A has no diagonal on the rows i % 11 == 7
ISOLATED = (37, 11)        # b_identity: the rows and columns i % 37 == 11 of A are empty


class Layout:
    """Which row plays which part (a function of N alone)."""

    def __init__(self, N):
        assert N >= 9
        self.N = N
        idx = np.arange(N)
        self.no_diag = idx[idx % NO_DIAG[0] == NO_DIAG[1]]
        self.isolated = idx[idx % ISOLATED[0] == ISOLATED[1]]
        plain = np.ones(N, bool)
        plain[[HUB, N - 1]] = False
        plain[self.no_diag] = False
        plain[self.isolated] = False
        cand = idx[plain & (idx > HUB)]                       # ladder rows: right of the hub, with a diagonal entry
        # spread over the rows, at most a third of them; lengths taken while the partners (free rows with a diagonal) suffice
        cand = cand[np.unique(np.linspace(0, len(cand) - 1, min(len(LADDER), N // 3)).astype(int))]
        self.ladder = {}
        for L, r in zip(LADDER, cand):
            partners = int(plain.sum()) - (len(self.ladder) + 1)
            if L - 2 > partners:
                break
            self.ladder[L] = int(r)
        self.loner = self.ladder[1]
        free = np.ones(N, bool)
        free[HUB] = False
        free[self.isolated] = False
        free[list(self.ladder.values())] = False
        self.free = idx[free]                                 # rows whose length is left alone (N - 1 among them)
        plain[list(self.ladder.values())] = False
        self.partners = idx[plain]                            # free rows with a diagonal, but for the last row


def ladder_lengths(N):
    return tuple(Layout(N).ladder)


def _sym(rows, cols, vals, N):
    """Symmetric matrix from strictly one-sided couplings (no duplicates among the unordered pairs)."""
    M = sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr()
    return M + M.T


def _patterns(N, seed):
    """Couplings as (rows, cols) with rows > cols or rows < cols, never both orders of a pair:
    hub, last column, A only / B only / both on the ladder rows, random A and random B among the free rows."""
    lay = Layout(N)
    rng = np.random.default_rng([seed, N])
    out = {}
    others = np.setdiff1d(np.arange(N), [HUB, lay.loner])
    out["hub"] = (np.full(len(others), HUB), others)
    fr = lay.free[lay.free != N - 1]
    last = fr[::5]
    last = last[last % NO_DIAG[0] != NO_DIAG[1]]
    out["last"] = (np.full(len(last), N - 1), last)
    a_only, b_only, both = [], [], []
    for L, r in lay.ladder.items():
        if L <= 2:
            continue
        cols = rng.choice(lay.partners, size=L - 2, replace=False)
        q = (L - 2) // 4
        b_only += [(r, c) for c in cols[:q]]
        both += [(r, c) for c in cols[q:2 * q]]
        a_only += [(r, c) for c in cols[2 * q:]]
    for key, lst in (("a_only", a_only), ("b_only", b_only), ("both", both)):
        arr = np.array(lst, dtype=int).reshape(-1, 2)
        out[key] = (arr[:, 0], arr[:, 1])
    # random couplings among the free rows (the last row has its own): i > j, and a no-diagonal row never on the j side
    taken = set(zip(*out["last"]))
    for key, per_row in (("a_rand", 3.0), ("b_rand", 1.5)):
        n = int(per_row * len(fr))
        i, j = rng.choice(fr, size=n), rng.choice(fr, size=n)
        i, j = np.maximum(i, j), np.minimum(i, j)
        keep = (i != j) & (j % NO_DIAG[0] != NO_DIAG[1])
        pairs = sorted(set(zip(i[keep].tolist(), j[keep].tolist())) - taken)
        arr = np.array(pairs, dtype=int).reshape(-1, 2)
        out[key] = (arr[:, 0], arr[:, 1])
    # one-sided couplings for the unsymmetric form: upper entries (i < j) and lower entries (i > j) on pairs of their own
    used = set(zip(*out["a_rand"])) | set(zip(*out["b_rand"]))
    for key in ("up", "low"):
        n = len(fr)
        i, j = rng.choice(fr, size=n), rng.choice(fr, size=n)
        i, j = np.maximum(i, j), np.minimum(i, j)
        keep = (i != j) & (j % NO_DIAG[0] != NO_DIAG[1])
        pairs = sorted(set(zip(i[keep].tolist(), j[keep].tolist())) - used - taken)
        used |= set(pairs)
        arr = np.array(pairs, dtype=int).reshape(-1, 2)
        if not len(arr):                                    # (N = 9: the symmetric couplings took every pair; one of them moves)
            i, j = out["a_rand"]
            arr = np.array([[i[-1], j[-1]]])
            out["a_rand"] = (i[:-1], j[:-1])
        out[key] = (arr[:, 1], arr[:, 0]) if key == "up" else (arr[:, 0], arr[:, 1])
    return lay, rng, out


def _clear(M, rows):
    """M without the rows and columns ``rows``."""
    keep = np.ones(M.shape[0])
    keep[rows] = 0.0
    D = sp.diags(keep)
    M = sp.csr_matrix(D @ M @ D)
    M.eliminate_zeros()
    return M


def _assemble(N, seed, b_identity, cplx, unsymmetric, integer):
    lay, rng, P = _patterns(N, seed)

    def vals(key, scale):
        n = len(P[key][0])
        if integer:
            v = rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n)
            return v.astype(float)
        return scale * rng.uniform(0.5, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)

    dA = np.arange(1, N + 1, dtype=float)
    if integer:
        dA = (np.arange(N) % 8 + 1.0) * np.where(np.arange(N) % 3 == 0, -1.0, 1.0)
    has = np.setdiff1d(np.arange(N), lay.no_diag)
    A = sp.coo_matrix((dA[has], (has, has)), shape=(N, N)).tocsr()
    # (B = I: the union pattern is A's, so A takes the couplings that are otherwise B's alone)
    for key, scale in (("hub", 0.01), ("last", 0.05), ("a_only", 0.05), ("both", 0.05), ("a_rand", 0.5)) + \
            ((("b_only", 0.05),) if b_identity else ()):
        A = A + _sym(*P[key], vals(key, scale), N)
    A = sp.csr_matrix(A)
    if unsymmetric:
        # the strictly lower part entry by entry by a factor of its own, then one-sided couplings
        low = sp.tril(A, -1).tocsr()
        f = rng.integers(1, 4, size=low.nnz).astype(float) if integer else rng.uniform(0.3, 0.9, size=low.nnz)
        low.data = np.clip(low.data * f, -8, 8) if integer else low.data * f
        A = sp.triu(A, 0).tocsr() + low
        for key in ("up", "low"):
            A = A + sp.coo_matrix((vals(key, 0.3), P[key]), shape=(N, N)).tocsr()
    if cplx:
        up = sp.triu(A, 1).tocoo()
        pick = np.random.default_rng([seed, N, 1]).random(up.nnz) < 0.5      # (a stream of its own: integer_pair gets the same pattern)
        n = int(pick.sum())
        im = (rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n)).astype(float) if integer else \
            0.3 * np.abs(up.data[pick]) * rng.choice([-1.0, 1.0], size=n)
        T = sp.coo_matrix((im, (up.row[pick], up.col[pick])), shape=(N, N)).tocsr()
        A = A + 1j * (T - T.T)
    A = sp.csr_matrix(A)
    if b_identity:
        A = _clear(A, lay.isolated)
        A.sort_indices()
        return A, None
    Boff = sp.csr_matrix((N, N))
    for key, scale in (("b_only", 0.2), ("both", 0.2), ("b_rand", 0.5)):
        Boff = Boff + _sym(*P[key], vals(key, scale), N)
    Boff = sp.csr_matrix(Boff)
    if integer:
        dB = (np.arange(N) % 5 + 1.0) * np.where(np.arange(N) % 2 == 0, -1.0, 1.0)
    else:
        dB = 4.0 + rng.random(N) + np.asarray(abs(Boff).sum(axis=1)).ravel()
    B = sp.csr_matrix(Boff + sp.diags(dB))
    if cplx and integer:
        up = sp.triu(B, 1).tocoo()
        im = (rng.integers(1, 9, size=up.nnz) * rng.choice([-1, 1], size=up.nnz)).astype(float)
        T = sp.coo_matrix((im, (up.row, up.col)), shape=(N, N)).tocsr()
        B = sp.csr_matrix(B + 1j * (T - T.T))
    A.sort_indices()
    B.sort_indices()
    return A, B


def ragged_pair(N, seed, b_identity=False, cplx=False, unsymmetric=False):
    """(A, B) as CSR (B None for b_identity), deterministic in the arguments; see the module text."""
    return _assemble(N, seed, b_identity, cplx, unsymmetric, False)


def integer_pair(N, seed, b_identity=False, cplx=False, unsymmetric=False):
    """The patterns of ragged_pair with integers in [-8, 8] (Gaussian integers under cplx; Hermitian unless
    unsymmetric).  B is no longer definite: this pair is for products, not for solves."""
    return _assemble(N, seed, b_identity, cplx, unsymmetric, True)


def integer_block(N, m, seed):
    """N x m block of Gaussian integers in [-16, 16], column-major complex128."""
    rng = np.random.default_rng([seed, N, m])
    X = rng.integers(-16, 17, size=(N, m)) + 1j * rng.integers(-16, 17, size=(N, m))
    return np.asfortranarray(X.astype(np.complex128))


def union_pattern(A, B):
    """The pattern the device stores: entries of A or B, explicit zeros included, as a CSR matrix of ones."""
    P = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    if B is not None:
        P = P + sp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
    P = sp.csr_matrix(P)
    P.sort_indices()
    return P
