"""The CSR product kernels (k_spmm, k_spmm_row, k_spmm_lds of fh_sparse.hip, the row gathers of fh_poly.hip) and the ingest
that feeds them (fh_ingest.hpp) on ragged sparsity patterns (ragged_cases.py): rows of 0, 1, 2, 7 .. 9, 15 .. 17, 24, 25,
31 .. 33, 64 and 65 entries and one of N - 1, rows without a diagonal, largest column on the diagonal or in the last
column, sizes that are multiples of nothing.

Exact comparisons.  integer_pair / integer_block hold integers: matrix entries in [-8, 8] (both parts), block entries in
[-16, 16].  One term of a row sum is below 2 * 8 * 16 = 256 in either part, a row has at most N <= 17000 entries, so
every product, every partial sum of a row in any order, and every value an FMA contraction forms before it rounds is an
integer below 2 * 256 * 17000 < 2^24 << 2^53: binary64 holds them all exactly and the device must return the integer
result bit for bit.  The tolerance of the products is therefore zero -- derived, not measured.  (scipy's product of the
same arrays is exact for the same reason: it is the integer result.)

Each test asserts that the path it names ran: the launches of the profile classes "spmm" / "spmm_adjoint" / "poly_spmm" /
"spmm_poly" (one per 64-column panel) and the device-side node counter of the gather kernels; the child processes of
test_other_kernels_on_the_same_data assert the renumbering line of FH_DEBUG_TIMING.  Which gather kernel a panel takes is
a function of (panel width, value type, FH_SPMM_ROW, FH_LDS_SPMM) alone (fh_apply_operator): real values at ld 64 take
k_spmm_row, everything else k_spmm, a renumbered matrix under FH_LDS_SPMM=1 k_spmm_lds.

A lane group of k_spmm takes a second row only when a slice has more than 128 x 16 rows (N > 4096 at ld 64): its
cross-row state (the far gather issued a row ahead, its refresh after a row without entries) cannot go wrong below that,
so the child that keeps the caller's row order also runs one product at N = 4400."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import ragged_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 21
SIZES = (9, 47, 331, 1003)
WIDTHS = (1, 16, 17, 32, 33, 64, 65, 100)           # ld 16, 32 and 64, one past each, and the m > 64 panel loop
FLAVOURS = {"real": {}, "hermitian": {"cplx": True}, "unsymmetric": {"unsymmetric": True},
            "unsymmetric-complex": {"cplx": True, "unsymmetric": True}}
U = 2.0 ** -53                                         # unit roundoff of binary64


def widths(N):
    return sorted(set(min(m, N) for m in WIDTHS))


def assert_exact_range(A, B, N):
    """The bound the zero tolerance rests on, checked on the data: no row sum comes near 2^53."""
    for M in (A, B):
        if M is not None:
            big = np.asarray((abs(M.real) + abs(M.imag)).sum(axis=1)).max()
            assert 2.0 * 16.0 * big < 2.0 ** 40, big


class Launches:
    """Launches of a profile class and node sweeps the gather kernels counted on the device, since the last look."""

    def __init__(self, eng, cls="spmm"):
        self.eng, self.cls = eng, cls
        eng.profile_enable(True)
        self.n, self.nodes = eng.profile_get(cls)[1], eng.profile_get("spmm.node_launches")[1]

    def take(self):
        n, nodes = self.eng.profile_get(self.cls)[1], self.eng.profile_get("spmm.node_launches")[1]
        d = (n - self.n, nodes - self.nodes)
        self.n, self.nodes = n, nodes
        return d


@pytest.fixture
def eng(engine):
    engine.set_adjoint(False)
    engine.require_adjoint(False)
    engine.set_solver("direct")
    engine.set_real_projection(False)
    yield engine
    engine.profile_enable(False)
    engine.set_adjoint(False)
    engine.require_adjoint(False)
    engine.set_solver("direct")
    engine.set_problem(np.eye(4))


# ---- a. exact products ---------------------------------------------------------------------------------------------------
def check_products(eng, N, flavour, bid, ms=None, lds=False):
    A, B = rc.integer_pair(N, SEED, b_identity=bid, **FLAVOURS[flavour])
    assert_exact_range(A, B, N)
    eng.set_problem(A, B)
    count = Launches(eng)
    Bm = sp.identity(N, format="csr") if B is None else B
    for m in ms or widths(N):
        X = rc.integer_block(N, m, m)
        dX = eng.upload(X)
        for which, M in ((0, A), (1, Bm)):
            Y = eng.download(eng.matmul(which, dX, m), m)
            want = np.asarray(M @ X)
            bad = np.argwhere(Y != want)
            assert np.array_equal(Y, want), "N=%d %s %s m=%d %s: %d entries differ, first (row, column) %s: %r for %r" % (
                N, flavour, "B=I" if bid else "B", m, "AB"[which], len(bad), bad[0], Y[tuple(bad[0])], want[tuple(bad[0])])
            launches, nodes = count.take()
            assert launches == (m + 63) // 64, (N, m, launches)                   # the CSR product, one launch per 64 columns
            assert lds or nodes == launches, (N, m, nodes)                        # a gather kernel (k_spmm_lds counts per block)


@pytest.mark.parametrize("bid", [False, True], ids=["B", "I"])
@pytest.mark.parametrize("flavour", ["real", "hermitian", "unsymmetric"])
@pytest.mark.parametrize("N", SIZES)
def test_products_are_the_integer_results(eng, N, flavour, bid):
    """engine.matmul(0 | 1) == A X, B X bit for bit for every width: k_spmm at ld 16, 32, 64 (complex values, or fewer than
    49 columns), k_spmm_row (real values, 49 .. 64 columns), the panel loop beyond 64.  B = I brings the rows without
    entries; N = 1003 is renumbered at ingest, the others are not."""
    check_products(eng, N, flavour, bid)


@pytest.mark.parametrize("N", SIZES)
def test_adjoint_products_are_the_integer_results(eng, N):
    """set_adjoint under solver "banded": A^H X and B^H X on the unsymmetric complex pencil, through the transposed CSR set
    (fh_adjoint_csr) and k_spmm.  A missed conjugate or an untransposed pattern changes integers."""
    A, B = rc.integer_pair(N, SEED, **FLAVOURS["unsymmetric-complex"])
    assert (A != A.conj().T).nnz and (rc.union_pattern(A, None) != rc.union_pattern(A, None).T).nnz    # unsymmetric in values and pattern
    eng.require_adjoint(True)
    eng.set_problem(A, B)
    eng.set_solver("banded")
    eng.set_adjoint(True)
    count = Launches(eng, "spmm_adjoint")
    for m in widths(N):
        X = rc.integer_block(N, m, m)
        dX = eng.upload(X)
        for which, M in ((0, A), (1, B)):
            Y = eng.download(eng.matmul(which, dX, m), m)
            assert np.array_equal(Y, np.asarray(M.conj().T @ X)), (N, m, which)
            assert count.take() == ((m + 63) // 64,) * 2


def test_rows_never_read_an_unknown_they_do_not_couple_to(eng):
    """One row of X is infinite.  Every row of A X and B X whose row of the stored (union) pattern has no entry in that
    column must come back as if it were zero: the padding slots of a chunk of 8 (k_spmm_row) and the lanes past the end of
    a row (k_spmm) point at the row itself and must not turn 0 * inf into NaN.  N = 331 keeps the caller's row order."""
    N, poisoned = 331, 0
    for bid in (False, True):
        A, B = rc.integer_pair(N, SEED, b_identity=bid)
        eng.set_problem(A, B)
        P = rc.union_pattern(A, B).tocsc()
        touched = np.zeros(N, bool)
        touched[P.indices[P.indptr[poisoned]:P.indptr[poisoned + 1]]] = True
        touched[poisoned] = True
        assert 3 <= touched.sum() <= N // 4
        for m in (17, 64):
            X = rc.integer_block(N, m, m)
            X0 = X.copy()
            X0[poisoned] = 0.0
            X[poisoned] = np.inf
            dX = eng.upload(X)
            for which, M in ((0, A), (1, sp.identity(N, format="csr") if B is None else B)):
                Y = eng.download(eng.matmul(which, dX, m), m)
                assert np.array_equal(Y[~touched], np.asarray(M @ X0)[~touched]), (bid, m, which)


def test_polynomial_products_are_the_integer_results(eng):
    """A CSR polynomial with the coefficients (ragged A, ragged B, an empty matrix): A_lin X and B_lin X of the companion
    form (poly_matmul) and P(z_e) X_e at Gaussian-integer nodes (poly_node_products), through the row gathers of fh_poly.hip
    in batches of 4.  |z| <= 4, so one entry of P(z) stays below 8 + 4 * 8 in either part and every sum far below 2^53."""
    import polynomial_reference as pr
    from feastkit_jl_amd.ingest import polynomial_union_csr
    N = 331
    A, B = rc.integer_pair(N, SEED, cplx=True)
    coeffs = [A, B, sp.csr_matrix((N, N))]
    Z = np.array([2.0 + 1.0j, -3.0 + 0.0j, 0.0 + 1.0j])
    eng.set_polynomial_csr(*polynomial_union_csr(coeffs))
    eng.set_solver("direct")
    eng.set_contour(Z, np.ones(3, dtype=complex), 1.0)
    Alin, Blin = pr.companion([c.toarray() for c in coeffs])
    count = Launches(eng, "poly_spmm")
    for m in (4, 17):
        X = rc.integer_block(2 * N, m, m)
        dX = eng.upload(X)
        for which, M in ((0, Alin), (1, Blin)):
            Y = eng.download(eng.poly_matmul(which, dX, m), m)
            assert np.array_equal(Y, M @ X), (m, which)
        assert count.take()[0] >= 1
    count = Launches(eng, "spmm_poly")
    for m in (7, 24, 64):
        X = [rc.integer_block(N, m, 10 * m + e) for e in range(3)]
        Y = eng.download(eng.poly_node_products(eng.upload(np.concatenate(X, axis=1)), m))
        for e, z in enumerate(Z):
            assert np.array_equal(Y[:, e * m:(e + 1) * m], np.asarray((A + z * B) @ X[e])), (m, e)
        assert count.take()[0] >= 1


# ---- b. exact residuals --------------------------------------------------------------------------------------------------
def check_residuals(eng, N, flavour, bid, rs=(7, 24, 64, 100)):
    """ritz_residual with V = I, integer lambda and normalize off: X = Q V is Q, R = A X - B X diag(lambda) holds integers,
    the squared column norms are integers below 2^53 and exact in any order, and the documented formula
    res_j = sqrt(sum_i |R_ij|^2) / max(|lambda_j|, 1) (fh_residual_norms) rounds twice: the square root and the division
    (|lambda_j| is an integer, the maximum is exact).  Both are correctly rounded operations of the host, so the result is
    within 2 u + u^2 (u = 2^-53) of the exact value, relatively; the reference below is formed in long double (error
    2^-63) and the bound asserted is 2.01 u."""
    A, B = rc.integer_pair(N, SEED, b_identity=bid, **FLAVOURS[flavour])
    eng.set_problem(A, B)
    Bm = sp.identity(N, format="csr") if B is None else B
    count = Launches(eng)
    for r in rs:
        r = min(r, N)
        Q = rc.integer_block(N, r, 7 * r)
        lam = (np.arange(r) % 7 - 3.0).astype(np.complex128)          # -3 .. 3, zero included
        dX, res = eng.ritz_residual(eng.upload(Q), r, np.eye(r), lam, r, normalize=False)
        assert np.array_equal(eng.download(dX, r), Q), (N, flavour, bid, r)
        R = np.asarray(A @ Q) - np.asarray(Bm @ Q) * lam[None, :]
        S = (R.real ** 2 + R.imag ** 2).sum(axis=0)
        assert S.max() < 2.0 ** 53
        want = np.sqrt(S.astype(np.longdouble)) / np.maximum(np.abs(lam), 1.0).astype(np.longdouble)
        err = np.abs(res.astype(np.longdouble) - want) / np.where(want > 0, want, 1)
        print("ragged-residual N=%d %s %s r=%d: largest relative error %.2f u" % (N, flavour, "I" if bid else "B", r, float(err.max() / U)))
        assert err.max() <= 2.01 * U, (N, flavour, bid, r, float(err.max() / U))
        launches, nodes = count.take()
        assert launches == (r + 63) // 64, (r, launches)


@pytest.mark.parametrize("N,flavour,bid", [(47, "real", True), (331, "real", False), (331, "hermitian", False), (331, "real", True),
                                           (1003, "real", False), (1003, "unsymmetric", True)])
def test_residuals_of_integer_blocks(eng, N, flavour, bid):
    """The per-column-coefficient form of the product (uniform_coef = 0: coefB = -lambda_j) on ragged rows."""
    check_residuals(eng, N, flavour, bid)


# ---- c. the other kernels on the same data -------------------------------------------------------------------------------
WORKER = r'''
import os, sys
sys.path[:0] = [r"{root}", r"{root}/oracle", r"{root}/tests"]
import feastkit_jl_amd as fk
import test_gpu_ragged_patterns as t
eng = fk.HipEngine(0)
lds = os.environ.get("FH_LDS_SPMM") == "1"
for N in (331, 1003):
    for flavour in ("real", "hermitian", "unsymmetric"):
        for bid in (False, True):
            t.check_products(eng, N, flavour, bid, lds=lds)
    for flavour, bid in (("real", False), ("hermitian", False), ("real", True)):
        t.check_residuals(eng, N, flavour, bid)
if os.environ.get("FH_REORDER") == "0":
    # caller's order, N > 4096: the lane groups of k_spmm at ld 64 take a second row 2048 further on, and the rows
    # 11, 48, 85, 122 (2211, ... in the other slice) have no entries while the rows 2048 after them have
    t.check_products(eng, 4400, "hermitian", True, ms=(64,))
eng.close()
print("ragged worker ok")
'''


@pytest.mark.parametrize("env", [{"FH_SPMM_ROW": "0"}, {"FH_REORDER": "2", "FH_LDS_SPMM": "1"}, {"FH_REORDER": "0"}],
                         ids=lambda e: "+".join("%s=%s" % kv for kv in e.items()))
def test_other_kernels_on_the_same_data(tmp_path, env):
    """The products and residuals above at N = 331 and N = 1003 in a fresh process under the switches that pick the other
    kernels: k_spmm for full-width real panels; ingest's renumbering into row blocks with k_spmm_lds (the hub row alone has
    N - 1 - 127 > 160 columns outside its block of at most 128 rows: the overflow slot 0xFFFF is used); the caller's row order."""
    assert min(331, 1003) - 1 - 127 > 160
    script = tmp_path / "ragged_worker.py"
    script.write_text(WORKER.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, FH_DEBUG_TIMING="1", **env), timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "ragged worker ok" in out, out[-4000:]
    assert ("renumbered into" in out) == (env.get("FH_REORDER") != "0"), out[-2000:]
