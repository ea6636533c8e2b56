"""feast_polynomial(..., solver="sparse_direct"), the host half: the union-pattern ingest against scipy, the analytic damped
cases and what the numpy restatement of the driver does on them (the expectation the device test is held to), and the
keyword validation, which touches no device."""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import polynomial_reference as pr
import polynomial_sparse_cases as sc
from feastkit_jl_amd.ingest import polynomial_union_csr


def _scatter(rowptr, col, v, N):
    return sp.csr_matrix((v, col, rowptr), shape=(N, N)).toarray()


def _check_union(coeffs):
    N = coeffs[0].shape[0]
    rowptr, col, vals = polynomial_union_csr(coeffs)
    assert rowptr.dtype == np.int64 and col.dtype == np.int64 and rowptr[0] == 0 and rowptr[-1] == len(col)
    assert len(vals) == len(coeffs) and all(v.shape == col.shape for v in vals)
    cplx = any(np.iscomplexobj(sp.csr_matrix(c).data) for c in coeffs)
    assert all(v.dtype == (np.complex128 if cplx else np.float64) for v in vals)
    # columns strictly increasing inside every row (what feasthip_set_polynomial_csr enforces), the whole diagonal present
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    same_row = rows[1:] == rows[:-1]
    assert np.all(col[1:][same_row] > col[:-1][same_row])
    assert np.count_nonzero(rows == col) == N
    # the pattern is the union of the coefficients' patterns and the diagonal, nothing more
    want = sp.identity(N, format="csr")
    for c in coeffs:
        c = sp.csr_matrix(c)
        want = want + sp.csr_matrix((np.ones(c.nnz), c.indices, c.indptr), shape=(N, N))
    assert len(col) == sp.csr_matrix(want).nnz
    # every coefficient is reproduced exactly, and so is P(z)
    dense = [np.asarray(sp.csr_matrix(c).toarray()) for c in coeffs]
    for k, v in enumerate(vals):
        assert np.array_equal(_scatter(rowptr, col, v, N), dense[k])
    for z in (0.3 - 0.7j, -1.1 + 0.2j):
        P = _scatter(rowptr, col, sum(z ** k * v for k, v in enumerate(vals)), N)
        ref = pr.poly_at(dense, z)
        assert np.abs(P - ref).max() <= 8 * np.finfo(float).eps * max(1.0, np.abs(ref).max())
    return rowptr, col, vals


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", sc.GRIDS[:2])
def test_union_pattern_of_the_mixed_coefficients(grid, d, cplx):
    coeffs = sc.mixed_pattern_coeffs(grid, d, cplx)
    patterns = {(tuple(c.indptr), tuple(c.indices)) for c in coeffs}
    assert len(patterns) >= min(d + 1, 3)                  # the patterns do differ
    if d >= 3:
        assert coeffs[2].nnz == 0                          # a coefficient without any entry
    assert np.any(np.diff(coeffs[1].indptr) == 0)          # rows that are empty in one coefficient
    if cplx and d >= 2:                                    # mixed real and complex input
        assert np.iscomplexobj(coeffs[1].data) and not np.iscomplexobj(coeffs[0].data)
    _check_union(coeffs)


def test_union_pattern_adds_a_missing_diagonal_and_sums_duplicates():
    N = 7
    A0 = sp.coo_matrix(([1.0, 2.0, 3.0, 4.0], ([0, 0, 2, 6], [1, 1, 5, 0])), shape=(N, N))          # (0, 1) twice: summed
    A1 = sp.csc_matrix(([5.0 + 1j, 6.0], ([3, 4], [3, 0])), shape=(N, N))                           # complex, CSC
    A2 = sp.csr_matrix((N, N))                                                                        # no entry
    rowptr, col, vals = _check_union([A0, A1, A2])
    # rows 1 and 5 are empty in every coefficient: the union holds their diagonal alone, with explicit zeros
    assert rowptr[2] - rowptr[1] == 1 and col[rowptr[1]] == 1 and all(v[rowptr[1]] == 0 for v in vals)
    assert vals[0][rowptr[0] + 1] == 3.0 and col[rowptr[0] + 1] == 1
    assert np.count_nonzero(vals[2]) == 0
    # float32 input is promoted by the ingest's float64 arrays
    r32, c32, v32 = polynomial_union_csr([sp.csr_matrix(A0, dtype=np.float32), sp.csr_matrix(A2, dtype=np.float32)])
    assert v32[0].dtype == np.float64 and v32[1].dtype == np.float64


@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES + [("20x16", True), ("24x18", False)])
def test_damped_cases_have_the_analytic_spectrum(name, scaled):
    case = sc.damped_case(name, scaled)
    assert len(case["lam_in"]) == case["k"]
    d = np.abs(case["lam_all"] - case["center"]) / case["radius"]
    print("farthest inside %.3f r, nearest outside %.3f r" % (d[d <= 1].max(), d[d > 1].min()))
    assert d[d <= 1].max() <= 0.9 and d[d > 1].min() >= 1.1
    coeffs = sc.dense(case["coeffs"])
    if scaled:
        assert np.iscomplexobj(coeffs[2]) and np.abs(coeffs[2] - np.eye(case["N"])).max() > 0.1        # non-monic, complex
    # the analytic values are eigenvalues: P(lambda) is singular to rounding
    for lam in case["lam_in"]:
        s = np.linalg.svd(pr.poly_at(coeffs, lam), compute_uv=False)
        assert s[-1] <= 1e-12 * s[0]


@pytest.mark.parametrize("seed", [20260515, 1, 2])
@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES, ids=sc.DRIVER_IDS)
def test_restatement_on_the_damped_cases(name, scaled, seed):
    """16 nodes, fpm[3] = 10: loops 4 (20 x 16) and 5 (24 x 18) for the three seeds, both sides of the last step clear of 1e-10."""
    case = sc.damped_case(name, scaled)
    run = pr.driver(sc.dense(case["coeffs"]), case["center"], case["radius"], case["M0"], ne=sc.NE, fpm3=sc.FPM3, seed=seed)
    hist = run["eps_hist"]
    print("loop %d history %s eigenvalue error %.2e backward error %.2e" % (
        run["loop"], ["%.1e" % e for e in hist], pr.match_error(run["lam"], case["lam_in"]), run["backward_error"].max()))
    assert run["info"] == 0 and run["M"] == case["k"]
    assert run["loop"] == case["loop"]
    if seed == 20260515:               # the start block of the device test: 5.5e-10 -> 3.3e-12 and 1.0e-9 -> 1.9e-11
        assert hist[-2] > 3e-10 and hist[-1] < 1e-10 / 3
    assert all(b < a for a, b in zip(hist[1:-1], hist[2:]))            # monotone once the subspace has formed
    assert pr.match_error(run["lam"], case["lam_in"]) <= 1e-12
    assert run["backward_error"].max() <= 1e-12


def test_saddle_quadratic_has_zero_diagonal_blocks_and_a_clear_circle():
    case = sc.saddle_quadratic()
    for c in case["coeffs"]:
        assert np.count_nonzero(c.diagonal() == 0) >= 99           # the pressures: structurally zero in every coefficient
    print("N %d, %d eigenvalues inside, gap %.2f r" % (case["N"], len(case["lam_in"]), case["gap"]))
    assert 3 <= len(case["lam_in"]) <= 8 and case["gap"] >= 0.1


def _sparse(n=6, count=3):
    rng = np.random.default_rng(5)
    return [sp.csr_matrix(rng.standard_normal((n, n))) for _ in range(count)]


@pytest.mark.parametrize("coeffs,kw,word", [
    (_sparse(), {"solver": "banded"}, "solver"),
    (_sparse(), {"solver": "lu"}, "solver"),
    ([c.toarray() for c in _sparse()], {"solver": "sparse_direct"}, 'solver="direct"'),
    (_sparse()[:2] + [_sparse()[2].toarray()], {"solver": "sparse_direct"}, 'solver="direct"'),
    (_sparse(), {"solver": "sparse_direct", "residual": "relative"}, "residual"),
])
def test_solver_keyword_validation_is_host_only(coeffs, kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    with pytest.raises(ValueError, match=word):
        fk.feast_polynomial(coeffs, 0.0, 1.0, M0=3, **kw)


def test_sparse_direct_takes_any_size_and_direct_keeps_its_window(monkeypatch):
    class Reached(Exception):
        pass

    def no_engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(fk.api, "_engine", no_engine)
    n = fk.api.POLY_DENSE_LIMIT + 1
    I = sp.identity(n, format="csr")
    with pytest.raises(Reached):
        fk.feast_polynomial([I, I, I], 0.0, 1.0, M0=3, solver="sparse_direct")
    with pytest.raises(ValueError, match="sparse"):
        fk.feast_polynomial([I, I, I], 0.0, 1.0, M0=3, solver="direct")
    with pytest.raises(Reached):
        fk.feast_polynomial(_sparse(), 0.0, 1.0, M0=3, solver="direct")


def test_symbol_is_declared():
    assert "feasthip_set_polynomial_csr" in fk.SYMBOLS
    assert fk.api.POLY_SOLVERS == ("direct", "sparse_direct")
