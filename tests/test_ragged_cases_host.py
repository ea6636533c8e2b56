"""ragged_cases.py on the host: the structural properties its text promises, for every (N, flags) the GPU tests use, so that a
later edit of the generator cannot lose one silently; the long-double row-sum product of krylov_reference.Pencil over rows
without entries; and, for every ragged entry of the step-exact case tables (krylov_cases, shifted_cases; gmres_cases is
covered by test_gmres_reference_host.py, which loops over its whole table), the conditions on the reference alone that the
device comparisons rest on: 32 D <= POWER, at most LEFT_OUT_MAX of the stops undecided, the fp64 restatement takes the
steps of the long-double one.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import krylov_cases as kc
import krylov_reference as kr
import ragged_cases as rc
import shifted_cases as sc
from test_gpu_primitives import sparse_pair

SEED = kc.RAGGED_SEED
FLAGS = [{}, {"b_identity": True}, {"cplx": True}, {"cplx": True, "b_identity": True}, {"unsymmetric": True},
         {"unsymmetric": True, "b_identity": True}, {"cplx": True, "unsymmetric": True}]
SIZES = (9, 47, 323, 331, 1003, 4400)
# the row lengths of the ladder that fit: the partners of a ladder row are rows with a diagonal that are on no ladder
FIT = {9: (1, 2), 47: rc.LADDER[:11]}


def _flag_id(f):
    return "+".join(sorted(f)) or "default"


@pytest.mark.parametrize("flags", FLAGS, ids=_flag_id)
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("make", [rc.ragged_pair, rc.integer_pair], ids=["ragged", "integer"])
def test_structure(make, N, flags):
    A, B = make(N, SEED, **flags)
    bid = flags.get("b_identity", False)
    assert sp.isspmatrix_csr(A) and A.shape == (N, N) and (B is None) == bid
    A2, B2 = make(N, SEED, **flags)
    assert (A != A2).nnz == 0 and np.array_equal(A.indices, A2.indices) and (bid or (B != B2).nnz == 0)     # deterministic
    assert N % 8 and N % 16 or N == 4400
    P = rc.union_pattern(A, B)
    length = np.diff(P.indptr)
    rows = np.repeat(np.arange(N), length)
    lay = rc.Layout(N)
    # row-length ladder
    assert tuple(lay.ladder) == FIT.get(N, rc.LADDER)
    for L, r in lay.ladder.items():
        assert length[r] == L, (L, r, length[r])
    # hub: every row but the loner (and the isolated ones)
    n_iso = len(lay.isolated) if bid else 0
    assert rc.HUB <= 8 and length[rc.HUB] == N - 1 - n_iso and length.max() == length[rc.HUB]
    assert P[:, rc.HUB].nnz == N - 1 - n_iso
    hub = np.asarray(abs(A[rc.HUB]).todense()).ravel()
    hub[rc.HUB] = 0.0
    if make is rc.ragged_pair:
        assert 0.0 < hub.max() <= 0.011                                             # weak couplings: the spectrum stays tame
    # largest column of a row: the diagonal, the last column, or left of the diagonal altogether
    largest = np.full(N, -1)
    np.maximum.at(largest, rows, P.indices)
    filled = length > 0
    assert (largest[filled] == np.arange(N)[filled]).sum() >= 2                     # no swap at ingest
    assert ((largest == N - 1) & (np.arange(N) < N - 1)).sum() >= (1 if N == 9 else 5)
    assert ((largest < np.arange(N)) & filled).sum() >= (1 if bid else 0) * (N > 9)  # neither a diagonal nor anything right of it
    # diagonal of A: missing on every 11th row, 1 .. N elsewhere
    d = A.diagonal()
    has = np.ones(N, bool)
    has[lay.no_diag] = False
    if bid:
        has[lay.isolated] = False
    assert len(lay.no_diag) in (N // 11, N // 11 + 1) and not d[~has].any()
    stored = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape).diagonal() > 0
    assert np.array_equal(stored, has)                                              # missing, not a stored zero
    if make is rc.ragged_pair:
        assert np.array_equal(d[has], np.arange(1, N + 1)[has])
    # isolated rows and columns
    if bid:
        assert len(lay.isolated) in (N // 37, N // 37 + 1) and rc.HUB not in lay.isolated
        assert np.array_equal(np.flatnonzero(length == 0), lay.isolated)
        assert not np.diff(A.tocsc().indptr)[lay.isolated].any()
        assert (N < 48) or len(lay.isolated) >= 1
    else:
        assert length.min() >= 1                                                    # with B the union has no empty row
    # B: symmetric, strictly diagonally dominant, a pattern of its own; union entries that are zero in A or in B
    if not bid:
        PA, PB = rc.union_pattern(A, None), rc.union_pattern(B, None)
        assert (PA != PB).nnz and (P - PA).nnz and (P - PB).nnz
        if make is rc.ragged_pair:
            assert abs(B - B.T).max() == 0.0
            off = np.asarray(abs(B).sum(axis=1)).ravel() - abs(B.diagonal())
            assert (B.diagonal() > off).all()
    # symmetry class
    if flags.get("unsymmetric"):
        PA = rc.union_pattern(A, None)
        assert (PA != PA.T).nnz and abs(A - A.T).max() > 0
    else:
        assert abs(A - A.conj().T).max() == 0.0
        assert np.iscomplexobj(A.data) == bool(flags.get("cplx"))
        if flags.get("cplx"):
            assert abs(A.imag).max() > 0 and (make is rc.ragged_pair or (B is None or abs(B - B.conj().T).max() == 0.0))
    if make is rc.integer_pair:
        for M in (A, B):
            if M is not None:
                v = M.data
                assert np.array_equal(v, np.round(v.real) + 1j * np.round(v.imag) if np.iscomplexobj(v) else np.round(v))
                assert max(abs(v.real).max(), abs(v.imag).max()) <= 8 and (v != 0).all()
        # the same patterns as ragged_pair
        Ar, Br = rc.ragged_pair(N, SEED, **flags)
        assert (rc.union_pattern(A, None) != rc.union_pattern(Ar, None)).nnz == 0
        assert bid or (rc.union_pattern(B, None) != rc.union_pattern(Br, None)).nnz == 0


def test_sizes_leave_slices_with_one_row_and_with_none():
    """N = 9 under the 8 row slices of ceil(N / 8) rows (k_spmm at ld 16, k_spmm_row): four slices of two rows, one of one,
    three of none; N = 1003 with the hub is renumbered at ingest by default (N >= 512, kl + ku > 512), N = 331 is not."""
    rows = -(-9 // 8)
    per = [max(0, min(9, (s + 1) * rows) - min(9, s * rows)) for s in range(8)]
    assert per.count(2) == 4 and per.count(1) == 1 and per.count(0) == 3
    for N in (331, 1003):
        P = rc.union_pattern(*rc.ragged_pair(N, SEED))
        r = np.repeat(np.arange(N), np.diff(P.indptr))
        assert (r - P.indices).max() + (P.indices - r).max() > 512
    assert 331 < 512 <= 1003


def test_integer_block():
    X = rc.integer_block(331, 17, 3)
    assert X.flags.f_contiguous and X.dtype == np.complex128 and X.shape == (331, 17)
    assert np.array_equal(X, np.round(X.real) + 1j * np.round(X.imag)) and abs(X.real).max() == 16 and abs(X.imag).max() == 16
    assert np.array_equal(X, rc.integer_block(331, 17, 3)) and not np.array_equal(X, rc.integer_block(331, 17, 4))


# ---- the long-double product over rows without entries --------------------------------------------------------------------
@pytest.mark.parametrize("flags", [{"b_identity": True}, {"b_identity": True, "cplx": True}, {}], ids=_flag_id)
def test_pencil_with_empty_rows_agrees_with_scipy(flags):
    N = 331
    A, B = rc.ragged_pair(N, SEED, **flags)
    if B is not None:
        B = sp.csr_matrix(sp.diags(np.where(np.arange(N) % 5 == 2, 0.0, 1.0)) @ B)     # B with rows without entries too
        B.eliminate_zeros()
    empty = np.flatnonzero(np.diff(A.indptr) == 0)
    assert len(empty) == (9 if flags.get("b_identity") else 0) and (B is None or (np.diff(B.indptr) == 0).sum() > 60)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    PL, PD = kr.Pencil(A, B, np.clongdouble), kr.Pencil(A, B, np.complex128)
    for mul, M in ((PL.mulA, A), (PL.mulB, B)):
        if M is None:
            assert np.array_equal(PL.mulB(x.astype(np.clongdouble)), x)
            continue
        y = mul(x.astype(np.clongdouble))
        assert y.dtype == np.clongdouble and y.shape == (N,)
        assert not y[np.diff(M.indptr) == 0].any()                                   # a zero for a row without entries
        ref = M @ x
        # rounding of the complex128 product: (row length + 2) eps sum |a_ij| |x_j| per row
        bound = (np.diff(M.indptr) + 2) * np.finfo(float).eps * (abs(M) @ abs(x))
        assert (np.abs(y.astype(np.complex128) - ref) <= bound).all()
    z = 0.3 + 0.2j
    got = PL.apply(z, x.astype(np.clongdouble))
    want = PD.apply(z, x)
    assert np.abs(got.astype(np.complex128) - want).max() <= 1e-13 * np.abs(want).max()
    if B is None:
        assert np.array_equal(got[empty], np.clongdouble(z) * x[empty].astype(np.clongdouble))    # that row of z I - A is z


def test_pencil_without_empty_rows_is_bitwise_what_it_was():
    A, _ = sparse_pair(45, 8, b_identity=True)
    M = A.tocsr()
    M.sort_indices()
    x = (np.random.default_rng(2).standard_normal(45) + 1j * np.random.default_rng(3).standard_normal(45)).astype(np.clongdouble)
    old = np.add.reduceat(M.data.astype(np.longdouble) * x[M.indices], M.indptr[:-1])     # the expression before empty rows
    new = kr.Pencil(A, None, np.clongdouble).mulA(x)
    assert new.dtype == old.dtype and np.array_equal(new, old)


# ---- the ragged entries of the step-exact tables: conditions on the reference alone ---------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("name", kc.RAGGED)
def test_truncated_ragged_inputs(name, near):
    c = kc.trunc_case(name, near)
    assert c.ks == (kc.TRUNC[name][5] if near else kc.TRUNC[name][4])
    for k in c.ks:
        print("ragged-host truncated/%s/%s/k=%d 32D=%.2e" % (name, "near" if near else "far", k, 32.0 * c.drift[k]))
        assert 32.0 * c.drift[k] <= kc.POWER, (name, near, k, c.drift[k])
        assert c.fp64_steps_agree[k], (name, near, k)
        undecided = sum(kr.truncated(r, k)[4] < kc.MARGIN_MIN for r in c.ref)
        assert undecided <= kc.LEFT_OUT_MAX * len(c.ref), (name, near, k, undecided)


def test_near_ks_of_the_ragged_cocg_cases_are_the_longest_prefix():
    """krylov_cases lists, next to the spectrum, the longest prefix of TRUNC_KS that keeps 32 D <= POWER: the next k fails."""
    solver, method, build, m, ks_far, ks_near, interval = kc.TRUNC["cocg-ragged-I-N47-m7"]
    assert ks_near == kc.TRUNC_KS[:len(ks_near)] and len(ks_near) < len(kc.TRUNC_KS)
    nxt = kc.TRUNC_KS[len(ks_near)]
    A, B = build()
    z = kc.near_shift(interval)
    X = kc.rand_block(47, m, 8)
    PL, PD = kr.Pencil(A, B, np.clongdouble), kr.Pencil(A, B, np.complex128)
    D = 0.0
    for j in range(m):
        ref = kr.solve_column(PL, z, X[:, j], method, 1e-14, 0.0, nxt)
        for chunks, seed in kr.DRIFT_ORDERS:
            d = kr.solve_column(PD, z, X[:, j], method, 1e-14, 0.0, nxt, dots=kr.Dots(47, chunks, seed))
            D = max(D, kr.rel_dist(d.x, ref.x))
    assert 32.0 * D > kc.POWER, D
    for name in ("cocg-ragged-B-N323-m64", "cocg-ragged-I-N331-m17"):
        assert kc.TRUNC[name][4] == kc.TRUNC[name][5] == kc.TRUNC_KS
    # far from the spectrum the same pencil ends at k = 33: at k = 48 > 47 unknowns long double has stopped, complex128 has not
    assert ks_far == kc.TRUNC_KS[:-1]
    steps64 = set()
    for j in range(m):
        ref = kr.solve_column(PL, kc.FAR_SHIFT, X[:, j], method, 1e-14, 0.0, 48)
        assert ref.steps == 47 and not ref.active
        steps64 |= {kr.solve_column(PD, kc.FAR_SHIFT, X[:, j], method, 1e-14, 0.0, 48, dots=kr.Dots(47, chunks, seed)).steps
                    for chunks, seed in kr.DRIFT_ORDERS}
    assert steps64 == {47, 48}, steps64


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("m", kc.RAGGED_SWEEP_M)
@pytest.mark.parametrize("rtol,maxit", kc.SWEEP_SETTINGS)
@pytest.mark.parametrize("kind", kc.SWEEP_KINDS[1:])
def test_ragged_sweep_inputs(kind, rtol, maxit, m, warm):
    c = kc.sweep_case("cocg_fused", rtol, maxit, m, warm, kind=kind)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= kc.LEFT_OUT_MAX * c.decided.size
    for real in (True, False):
        print("ragged-host sweep/%s/rtol=%g/maxit=%d/m=%d/%s/%s 32D=%.2e" % (kind, rtol, maxit, m, "ritz" if warm else "zero",
                                                                          "real" if real else "complex", 32.0 * c.drift[real]))
        assert 32.0 * c.drift[real] <= kc.POWER, (kind, rtol, maxit, m, warm, real, c.drift[real])
    lo, hi = kc._SWEEP_INTERVAL[kind]
    ritz = kc.sweep_ritz(m, kind)
    assert ritz.min() < lo and ritz.max() > hi and ((ritz > lo) & (ritz < hi)).any()          # the guesses straddle the interval


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("m", [sc.LD_M[32], sc.LD_M[64]])
@pytest.mark.parametrize("rtol,maxit", sc.INEXACT)
@pytest.mark.parametrize("family", ["3", "16"])
def test_ragged_shifted_inputs(family, rtol, maxit, m, warm):
    c = sc.sweep_case(sc.RAGGED, family, rtol, maxit, m, warm)
    assert c.fp64_steps_agree and c.decided.all()
    print("ragged-host shifted/family=%s/rtol=%g/maxit=%d/m=%d/%s 32D=%.2e" % (family, rtol, maxit, m, "ritz" if warm else "zero",
                                                                             32.0 * max(c.drift.values())))
    assert 32.0 * max(c.drift.values()) <= sc.POWER, c.drift
    assert len(set(c.ref.steps.ravel())) >= 3                                                    # the nodes freeze at different steps
