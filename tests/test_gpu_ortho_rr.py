"""GPU tests of the staged rank-revealing Cholesky-QR (feasthip_set_ortho_method(FEASTHIP_ORTHO_CHOLQR_RR): k_pchol_stage
and the stage loop of fh_ortho_staged) against scipy's column-pivoted QR, the numpy restatement
(tests/cholqr_rr_reference.py) and the column-pivoted Gram-Schmidt on the same panels (tests/cholqr_rr_cases.py)."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import feastkit_jl_amd as fk
from feastkit_jl_amd import workloads

import cholqr_rr_cases as cs
import cholqr_rr_reference as rr

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(float).eps)
SHAPES = [(300, 1), (301, 16), (517, 32), (1000, 64), (4096, 64), (333, 23), (700, 47)]


def load(engine, N):
    engine.set_problem(sp.identity(N, format="csr") * 2.0, None)


def run(engine, X, method, ref=0.0, n_report=64):
    """orthonormalise X (N x m) by `method` -> (rank, Q, report)"""
    engine.set_ortho_method(method)
    try:
        m = X.shape[1]
        dQ = engine.upload(np.asfortranarray(X))
        rank = engine.orthonormalize(dQ, m, cs.SQRT_EPS)
        rep = engine.last_ortho(n_report)
        return rank, engine.download(dQ)[:, :rank].copy(), rep
    finally:
        engine.set_ortho_method("mgs")


@pytest.mark.parametrize("kind", [k for k in cs.KINDS if k != "f"])
@pytest.mark.parametrize("N,m", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_staged_path_against_scipy_numpy_and_gram_schmidt(engine, kind, N, m, cplx):
    X, _ = cs.make_case(kind, N, m, cplx, 1000 + m)
    rank_ref, piv, rd, r11, thr = cs.assert_unambiguous(X, cs.SQRT_EPS)
    load(engine, N)
    rank_m, Qm, rep_m = run(engine, X, "mgs")
    rank, Q, rep = run(engine, X, "cholqr_rr")
    assert rank == rank_ref == rank_m == rep["rank"]
    nX = np.linalg.norm(X)
    # the fast path's decision does not depend on the method: full-rank panels (all of kind a, every single column) take it
    # under both settings, rank-deficient ones never do
    assert (rep["method"] == "cholqr") == (rep_m["method"] == "cholqr")
    assert rep["method"] == ("cholqr" if kind == "a" or m == 1 else "cholqr_rr")
    if rep["method"] == "cholqr":
        assert rep["stages"] == 0 and rep["fell_back"] == 0 and rank == m
        assert np.array_equal(Q, Qm)                      # bit for bit
    else:
        assert rank < m and rep["fell_back"] == 0 and 1 <= rep["stages"] <= rr.MAX_STAGES
        assert rep_m["method"] == "mgs"
        want = rr.staged_qr(X, cs.SQRT_EPS)
        assert want["rank"] == rank
        np.testing.assert_allclose(rep["rdiag"][:rank], want["rdiag"], rtol=1e-6)
        for k in range(rank):         # the same pivot wherever the neighbours differ by more than 1e-6 relative
            lo, hi = max(0, k - 1), min(rank - 1, k + 1)
            clear = all(abs(want["rdiag"][j] - want["rdiag"][k]) > 1e-6 * want["rdiag"][k] for j in (lo, hi) if j != k)
            if clear:         # (an exact copy of the column is the same pivot: fixture d's duplicates tie at every step)
                assert rep["perm"][k] == want["perm"][k] or np.array_equal(X[:, rep["perm"][k]], X[:, want["perm"][k]]), \
                    (k, rep["perm"][:rank], want["perm"])
        assert sorted(rep["perm"][:rank]) == sorted(set(rep["perm"][:rank]))
        assert np.all(rep["perm"][rank:] == -1)
        # two runs of the staged path: the same bits
        rank2, Q2, rep2 = run(engine, X, "cholqr_rr")
        assert rank2 == rank and np.array_equal(Q2, Q) and np.array_equal(rep2["rdiag"], rep["rdiag"])
    if rank:
        defect = np.abs(Q.conj().T @ Q - np.eye(rank)).max()
        defect_m = np.abs(Qm.conj().T @ Qm - np.eye(rank)).max()
        print("defect staged %.3e gram-schmidt %.3e" % (defect, defect_m))
        assert defect <= 4.0 * defect_m + 1e-14
        Qs, _, _ = sla.qr(X, mode="economic", pivoting=True)
        Qs = Qs[:, :rank]
        res = np.linalg.norm(X - Q @ (Q.conj().T @ X))
        res_s = np.linalg.norm(X - Qs @ (Qs.conj().T @ X))
        print("residual staged %.3e scipy %.3e" % (res, res_s))
        assert res <= 4.0 * res_s + EPS * m * nX


@pytest.mark.parametrize("m", [1, 16, 64])
def test_all_zero_panel_has_rank_zero(engine, m):
    load(engine, 300)
    rank, Q, rep = run(engine, np.zeros((300, m), dtype=complex), "cholqr_rr")
    assert rank == 0 and rep["rank"] == 0 and rep["method"] == "cholqr_rr" and rep["fell_back"] == 0


def test_non_finite_panel_falls_back_to_gram_schmidt(engine):
    """a NaN in one column (the input of test_gpu_abi_errors.py): the staged path gives up on the non-finite Gram matrix and
    the Gram-Schmidt runs on the untouched panel, so the result is the default method's bit for bit"""
    N, m = 400, 8
    X = np.random.default_rng(5).standard_normal((N, m)) + 0j
    X[3, 2] = np.nan
    load(engine, N)
    engine.set_ortho_method("mgs")
    d0 = engine.upload(np.asfortranarray(X))
    rank0 = engine.orthonormalize(d0, m, cs.SQRT_EPS)
    Q0 = engine.download(d0).copy()
    rep0 = engine.last_ortho(m)
    engine.set_ortho_method("cholqr_rr")
    try:
        d1 = engine.upload(np.asfortranarray(X))
        rank1 = engine.orthonormalize(d1, m, cs.SQRT_EPS)
        Q1 = engine.download(d1).copy()
        rep1 = engine.last_ortho(m)
    finally:
        engine.set_ortho_method("mgs")
    assert rep0["fell_back"] == 0 and rep1["fell_back"] == 1 and rep1["method"] == "mgs" and rep1["stages"] == 0
    assert rank1 == rank0 and np.array_equal(rep1["perm"], rep0["perm"])
    assert np.array_equal(Q1.view(np.uint64), Q0.view(np.uint64))


def test_invalid_method_is_an_fpm_error(engine):
    lib = fk.load_library()
    for bad in (-1, 2, 7):
        assert lib.feasthip_set_ortho_method(engine.h, bad) == 9          # FEASTHIP_ERROR_FPM
    assert lib.feasthip_set_ortho_method(None, 0) == 7
    with pytest.raises(ValueError):
        engine.set_ortho_method("householder")
    assert lib.feasthip_last_ortho(engine.h, None, None, None, None, None, None, 0) == 0


@pytest.mark.parametrize("N,m,true_rank,cplx", [(600, 80, 50, True), (900, 129, 129, False), (800, 129, 70, True), (500, 80, 64, False)])
def test_wide_panels(engine, N, m, true_rank, cplx):
    """M0 > 64: 64-column blocks against the columns kept so far, ref_scale and the total width honoured"""
    rng = np.random.default_rng(N + m)
    basis = rng.standard_normal((N, true_rank)) + (1j * rng.standard_normal((N, true_rank)) if cplx else 0)
    mix = rng.standard_normal((true_rank, m)) + 0j
    X = basis @ mix if true_rank < m else basis + 0j
    rank_ref = cs.assert_unambiguous(X, cs.SQRT_EPS)[0]
    assert rank_ref == true_rank
    load(engine, N)
    rank_m, Qm, rep_m = run(engine, X, "mgs")
    rank, Q, rep = run(engine, X, "cholqr_rr")
    assert rank == rank_m == true_rank == rep["rank"] and rep["fell_back"] == 0
    if true_rank < m:
        assert rep["method"] == "cholqr_rr" and rep["stages"] >= 1
    else:
        assert np.array_equal(Q, Qm)
    defect = np.abs(Q.conj().T @ Q - np.eye(rank)).max()
    defect_m = np.abs(Qm.conj().T @ Qm - np.eye(rank)).max()
    print("defect staged %.3e gram-schmidt %.3e" % (defect, defect_m))
    assert defect <= 4.0 * defect_m + 1e-14
    Qs = sla.qr(X, mode="economic", pivoting=True)[0][:, :rank]
    res, res_s = np.linalg.norm(X - Q @ (Q.conj().T @ X)), np.linalg.norm(X - Qs @ (Qs.conj().T @ X))
    print("residual staged %.3e scipy %.3e" % (res, res_s))
    assert res <= 4.0 * res_s + EPS * m * np.linalg.norm(X)


@pytest.mark.parametrize("cplx", [False, True])
def test_block_of_a_wider_matrix(engine, cplx):
    """fixture f: the last 64-column block of a 128-column matrix whose first block has columns 1e5 times longer -- the
    threshold follows the R_11 of the whole matrix, so the second block, full rank on its own, loses its short columns"""
    N, m = 700, 64
    Xb, ref = cs.make_case("f", N, m, cplx, 77)
    rng = np.random.default_rng(78)
    lead = np.linalg.qr(rng.standard_normal((N, 64)))[0] * ref           # orthogonal columns of norm ref_scale
    Xb = Xb - lead @ (lead.T @ Xb) / ref ** 2                             # the block is what the projection leaves
    X = np.hstack([lead.astype(complex), Xb])
    rank_ref = cs.assert_unambiguous(X, cs.SQRT_EPS)[0]
    rank_blk = cs.assert_unambiguous(Xb, cs.SQRT_EPS, ref, 128)[0]
    assert rank_ref == 64 + rank_blk and rank_blk < cs.assert_unambiguous(Xb, cs.SQRT_EPS)[0]
    load(engine, N)
    rank_m, Qm, _ = run(engine, X, "mgs")
    rank, Q, rep = run(engine, X, "cholqr_rr")
    assert rank == rank_m == rank_ref and rep["fell_back"] == 0 and rep["method"] == "cholqr_rr"
    want = rr.staged_qr(Xb, cs.SQRT_EPS, ref, 128)
    assert want["rank"] == rank_blk
    assert np.abs(Q.conj().T @ Q - np.eye(rank)).max() <= 4.0 * np.abs(Qm.conj().T @ Qm - np.eye(rank)).max() + 1e-14


def test_resident_reduce_agrees_between_methods(engine):
    """feasthip_rr_reduce_resident on a resident Q_proj of rank 9 in 20 columns under both methods"""
    N, m = 900, 20
    rng = np.random.default_rng(4)
    A = sp.diags([np.arange(1.0, N + 1), -0.3 * np.ones(N - 1), -0.3 * np.ones(N - 1)], [0, 1, -1]).tocsr()
    B = sp.diags([4.0 + rng.random(N)], [0]).tocsr()
    engine.set_problem(A, B)
    src = np.asfortranarray((rng.standard_normal((N, 9)) + 1j * rng.standard_normal((N, 9))) @ (rng.standard_normal((9, m)) + 0j))
    out = {}
    for method in ("mgs", "cholqr_rr"):
        engine.set_ortho_method(method)
        try:
            engine.import_resident(engine.upload(src), m, which=1)
            rank, Sq, Aq = engine.rr_reduce_resident(m, cs.SQRT_EPS)
            rep = engine.last_ortho()
        finally:
            engine.set_ortho_method("mgs")
        assert rank == 9 and rep["method"] == method and rep["rank"] == 9
        out[method] = sla.eigh(Sq, Aq, eigvals_only=True)
    assert np.abs(out["mgs"] - out["cholqr_rr"]).max() <= 1e-10 * np.abs(out["mgs"]).max()


def test_feast_direct_end_to_end(engine):
    """the reduced cfg 3 through the sparse direct solver: every loop orthonormalises a rank-deficient Q_proj"""
    A, B, _ = workloads.laplacian_3d_pencil(30, 20, 12)
    out = {}
    for ortho in ("mgs", "cholqr_rr"):
        out[ortho] = fk.feast(A, B, (0.0, 0.25), M0=40, solver="direct", ortho=ortho, engine=engine)
    a, b = out["mgs"], out["cholqr_rr"]
    assert a.info == b.info == 0 and a.M == b.M > 0 and a.loop == b.loop
    assert np.abs(np.sort(a.lambda_) - np.sort(b.lambda_)).max() <= 1e-10
    for r in (a, b):
        R = A @ r.q - (B @ r.q) * r.lambda_[None, :]
        res = np.linalg.norm(R, axis=0) / np.maximum(np.abs(r.lambda_), 1.0) / np.linalg.norm(r.q, axis=0)
        assert res.max() <= 1e-10
    assert len(b.stats["ortho"]) == b.loop + 1 and len(a.stats["ortho"]) == a.loop + 1
    for entry in b.stats["ortho"]:
        assert entry["method"] == "cholqr_rr" and entry["stages"] >= 2 and entry["fell_back"] == 0
    assert all(e["method"] == "mgs" for e in a.stats["ortho"])
    assert [e["rank"] for e in a.stats["ortho"]] == [e["rank"] for e in b.stats["ortho"]]
    with pytest.raises(ValueError):
        fk.feast(A, B, (0.0, 0.25), M0=40, ortho="qr", engine=engine)


def test_feast_general_end_to_end(engine):
    """a small dense non-normal pencil: variant C never orthonormalises, so the keyword changes nothing it computes"""
    rng = np.random.default_rng(12)
    n = 120
    A = np.diag(np.linspace(-2.0, 2.0, n)) + 0.05 * rng.standard_normal((n, n))
    out = {o: fk.feast_general(A, None, 0.0, 0.6, M0=48, ortho=o, engine=engine) for o in ("mgs", "cholqr_rr")}
    a, b = out["mgs"], out["cholqr_rr"]
    assert a.info == b.info == 0 and a.M == b.M > 0 and a.loop == b.loop
    key = lambda r: np.lexsort((r.lambda_.imag.round(8), r.lambda_.real.round(8)))
    assert np.abs(a.lambda_[key(a)] - b.lambda_[key(b)]).max() <= 1e-10
    for r in (a, b):
        R = A @ r.q - r.q * r.lambda_[None, :]
        assert (np.linalg.norm(R, axis=0) / np.linalg.norm(r.q, axis=0)).max() <= 1e-10
    assert b.stats["ortho"] == []
