"""Term-operator handles (feasthip_set_term_operator, engine.set_term_operator, csrc/fh_termop.hip) on the device: the split
form T(z) X = sum_k f_k(z) A_k X on the caller's products, under the Krylov solvers.  Inputs and references:
term_operator_cases.py; the conditions on the references alone: test_term_operator_host.py.

Products are compared with the long-double product within 16 N eps (sum_k |F_k| ||A_k||_F) ||X||_F; truncated solves and sweeps
with the step-exact restatements (krylov_reference.py, gmres_reference.py on term_operator_cases.TermOp) within
krylov_reference.tolerance(D), D measured at test time; the drivers with the inexact restatement of feast_nonlinear under the
rules of test_gpu_nonlinear._check.  The callbacks multiply by dense torch copies of the test matrices."""
import numpy as np
import pytest

import feast_oracle as fo
import feastkit_jl_amd as fk
import gmres_cases as gc
import krylov_cases as kc
import krylov_reference as kr
import nonlinear_reference as nr
import operator_cases as oc
import polynomial_krylov_reference as pkr
import polynomial_projected_reference as ppr
import polynomial_sparse_cases as sc
import term_operator_cases as tc
from test_gpu_krylov_steps import check_sweep as krylov_check_sweep, close_enough
from test_gpu_nonlinear import _check, _fpm

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SOLVER_NAMES = ("FEASTHIP_SOLVER_BICGSTAB", "_GMRES", "_COCG")


@pytest.fixture(autouse=True)
def restore(engine, monkeypatch):
    """Leave the shared engine with an ordinary pencil and its default switches."""
    monkeypatch.delenv("FH_GMRES_BUDGET_MB", raising=False)
    yield
    engine.set_problem(np.eye(4))
    engine.set_adjoint(False)
    engine.set_node_solver(None)
    engine.set_solver("direct")
    engine.set_ortho_method("mgs")
    engine.set_real_projection(False)


def _install(engine, mats, funcs=None, contour=None, real=True, symmetric=False, muls=None, **kw):
    """The term-operator handle of these matrices; with a contour: its node values too."""
    engine.set_term_operator(tc.next_n(mats), tc.term_muls(engine, mats, real) if muls is None else muls, real=real, symmetric=symmetric, **kw)
    engine.set_real_projection(False)
    if contour is not None:
        engine.set_contour(contour[0], contour[1], 1.0)
        engine.nep_set_node_values(nr.table(funcs, contour[0]))


def _calls(engine, before):
    return [a - b for a, b in zip(engine.operator_stats()["term_calls"], before["term_calls"])]


# ---- 1. products -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real-view", "complex"])
@pytest.mark.parametrize("nt", [2, 3, 9])
@pytest.mark.parametrize("m", [7, 24, 40, 72])
def test_products(engine, m, nt, cplx):
    """engine.nep_eval_cols at N = 63 (a multiple of no tile; 95 for m = 72: two panels) for ld = 16, 32, 64: a unit-row table
    produces ONE term -- one callback per panel, none for the identity term -- and a random finite table all of them."""
    N = 63 if m <= 63 else 95
    mats, X, F = tc.product_inputs(N, m, nt, cplx)
    _install(engine, mats, real=not cplx)
    dX = engine.upload(X)
    panels = (m + 63) // 64
    for k in sorted({0, 1, nt - 1}):
        Fk = np.zeros((m, nt), dtype=np.complex128)
        Fk[:, k] = 1.0
        before = engine.operator_stats()
        R = engine.download(engine.nep_eval_cols(dX, Fk, m), m)
        ref, bound = tc.product_reference(mats, Fk, X)
        err = float(np.linalg.norm(R.astype(np.clongdouble) - ref))
        print("term product N=%d m=%d nt=%d unit row %d %s: error %.3e bound %.3e" % (N, m, nt, k, "complex" if cplx else "real", err, bound))
        assert err <= bound
        assert _calls(engine, before) == [panels if (j == k and mats[j] is not None) else 0 for j in range(nt)]
    before = engine.operator_stats()
    R = engine.download(engine.nep_eval_cols(dX, F, m), m)
    ref, bound = tc.product_reference(mats, F, X)
    err = float(np.linalg.norm(R.astype(np.clongdouble) - ref))
    print("term product N=%d m=%d nt=%d random table %s: error %.3e bound %.3e" % (N, m, nt, "complex" if cplx else "real", err, bound))
    assert err <= bound
    assert _calls(engine, before) == [0 if M is None else panels for M in mats]


@pytest.mark.parametrize("cplx", [False, True], ids=["real-view", "complex"])
def test_product_where_the_combine_loop_takes_a_second_trip(engine, cplx):
    """N = 6007, m = 40 (ld = 64): N ld = 384 448 elements against the grid limit of 1024 workgroups x 256 threads = 262 144
    (fh_op_combine_nblk), so half of the workgroups take a second trip of the grid-stride loop.  Matrix-free banded terms
    (operator_cases.band_mul) around an identity term."""
    N, m = 6007, 40
    mul, host, fro = oc.band_mul(engine, N, cplx)
    X = kc.rand_block(N, m, 3)
    rng = np.random.default_rng(5)
    F = rng.standard_normal((m, 3)) + 1j * rng.standard_normal((m, 3))
    engine.set_term_operator(N, [mul, None, mul], real=not cplx)
    before = engine.operator_stats()
    R = engine.download(engine.nep_eval_cols(engine.upload(X), F, m), m)
    ct = np.clongdouble
    ref = host(X * F[None, :, 0]) + X.astype(ct) * F[None, :, 1].astype(ct) + host(X * F[None, :, 2])
    per_col = (np.abs(F) @ np.array([fro, np.sqrt(N), fro])) * np.linalg.norm(X, axis=0)
    err, bound = float(np.linalg.norm(R.astype(ct) - ref)), 16.0 * N * EPS * float(np.linalg.norm(per_col))
    print("term product N=%d m=%d: error %.3e bound %.3e" % (N, m, err, bound))
    assert err <= bound
    assert _calls(engine, before) == [1, 0, 1]


# ---- 2. truncated solves are the k-th iterate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("solver", ["bicgstab", "cocg", "gmres"])
def test_truncated_solve_is_the_kth_iterate(engine, solver, near):
    """engine.nep_solve on the grid delay operator (N = 120, every term symmetric, the middle one the identity) at a node next
    to the spectrum and one far from it, maxit = k, rtol = 1e-14: the iterate within tolerance(D), return code and step counts
    by the rules of test_gpu_operator.test_truncated_solve_is_the_kth_iterate, for GMRES the products too."""
    mats, funcs, Z, W, _ = tc.grid_operator()
    c = tc.gmres_case(near) if solver == "gmres" else tc.trunc_case(solver, near)
    _install(engine, mats, funcs, (Z, W), symmetric=True)
    dX = engine.upload(c.X)
    for k in c.ks:
        kw = {"restart": c.restart} if solver == "gmres" else {}
        engine.set_solver(solver, rtol=1e-14, atol=0.0, maxit=k, **kw)
        dY, rc = engine.nep_solve(c.node, dX, c.m)
        Y = engine.download(dY)
        st = engine.last_stats
        want = c.want[k] if solver == "gmres" else [kr.truncated(r, k) for r in c.ref]      # (x, steps, status, active, margin)
        decided = [w[4] >= tc.MARGIN_MIN for w in want]
        assert sum(not d for d in decided) <= tc.LEFT_OUT_MAX * len(want)
        if all(decided):
            assert rc == (kr.NO_CONVERGENCE if any(w[3] for w in want) else 0), (solver, k, rc)
            if solver == "gmres":
                if any(w[1] == k for w in want):
                    assert st["krylov_iterations"] == k, (k, st)
                    assert st["spmm_calls"] == c.products[k], (k, st, c.products[k])
            else:
                assert st["krylov_iterations"] == (k if any(w[3] for w in want) else max(w[1] for w in want)), (solver, k, st)
            assert st["factorizations"] == 0
        dist = max(kr.rel_dist(Y[:, j], w[0]) for j, (w, ok) in enumerate(zip(want, decided)) if ok)
        close_enough("term-operator/truncated/%s/%s/k=%d" % (solver, "near" if near else "far", k), dist, c.drift[k])


# ---- 3. sweeps with mixed stops ------------------------------------------------------------------------------------------------------
def _run_sweep(engine, c, **kw):
    ne, m = len(c.Z), tc.SWEEP_M
    _install(engine, c.mats, c.funcs, (c.Z, c.W), symmetric=True, **kw)
    engine.set_solver(c.solver, rtol=c.rtol, atol=0.0, maxit=c.maxit)
    dQ, status, st = engine.nep_resinv_apply(engine.upload(c.X), m, c.sigma, None if c.sigma is None else nr.table(c.funcs, c.sigma))
    return engine.download(dQ, m), status, st, engine.last_column_iterations(ne, m), engine.last_node_iterations(ne)


@pytest.mark.parametrize("setting,shifted", tc.SWEEP_PARAMS, ids=pkr.case_id)
def test_inexact_sweep(engine, setting, shifted):
    """engine.nep_resinv_apply, 16 nodes, m = 8, plain and shifted: the summed block, the per-node status (5 where the cap
    bites), the per-column step counts over the decided pairs and the node counts equal the restatement's."""
    c = tc.sweep_case(setting, shifted)
    out, status, st, counts, node_its = _run_sweep(engine, c)
    assert st["factorizations"] == 0
    krylov_check_sweep("term-operator/sweep/%s" % pkr.case_id((setting, shifted)), c, out, status, False, counts, node_its, st)


def test_sweep_in_node_chunks_of_three_is_the_same_block(engine):
    """scratch_bytes for three nodes of two product panels: the callback sees nodes = 3 (and 1: the last chunk, and the
    right-hand side's evaluation), never 16, and the block is the unchunked one bit for bit."""
    c = tc.sweep_case(tc.SWEEPS[0], True)
    whole = _run_sweep(engine, c)
    seen = []

    def watching(mul):
        def f(Y, X):
            seen.append(X.shape[0])
            for e in range(X.shape[0]):
                mul(Y[e], X[e])
        return f
    muls = [None if M is None else watching(oc.matrix_mul(engine, M)) for M in c.mats]
    per_node = 2 * c.X.shape[0] * 16 * 16          # nt' = 2 panels of N x ld complex128, ld = 16
    chunked = _run_sweep(engine, c, muls=muls, batched=True, scratch_bytes=3 * per_node)
    assert set(seen) == {3, 1} and seen.count(1) < seen.count(3), sorted(set(seen))
    assert np.array_equal(chunked[0], whole[0])
    assert list(chunked[1]) == list(whole[1]) and np.array_equal(chunked[3], whole[3]) and list(chunked[4]) == list(whole[4])


def test_gmres_sweep_in_node_batches_of_three(engine, monkeypatch):
    """The 16-node plain GMRES sweep under FH_GMRES_BUDGET_MB batches of 3: the callback sees nodes = 3 and 1; every solve passes
    the stop test, so the block lies within 2 rtol ||X|| sum_e |w_e| ||T(z_e)^-1||_2 of the exact-solve sweep
    (test_gpu_polynomial_krylov._converged_sweep_check's bound)."""
    rtol, maxit, restart = tc.GMRES_SWEEP
    mats, funcs, Z, W, X, _ = tc.sweep_inputs()
    seen = []

    def watching(mul):
        def f(Y, Xp):
            seen.append(Xp.shape[0])
            for e in range(Xp.shape[0]):
                mul(Y[e], Xp[e])
        return f
    muls = [None if M is None else watching(oc.matrix_mul(engine, M)) for M in mats]
    _install(engine, mats, funcs, (Z, W), symmetric=True, muls=muls, batched=True)
    engine.set_solver("gmres", rtol=rtol, atol=0.0, maxit=maxit, restart=restart)
    monkeypatch.setenv("FH_GMRES_BUDGET_MB", str(gc.budget_mb(X.shape[0], tc.SWEEP_M, restart, tc.GMRES_BATCH)))
    dQ, status, st = engine.nep_resinv_apply(engine.upload(X), tc.SWEEP_M)
    assert set(seen) == {3, 1} and not status.any() and st["krylov_iterations"] > 0 and st["factorizations"] == 0
    T = [tc.dense_t(mats, funcs, z, np.complex128) for z in Z]
    want = sum(w * np.linalg.solve(Te, X) for w, Te in zip(W, T))
    bound = 2.0 * rtol * np.linalg.norm(X) * sum(abs(w) * np.linalg.norm(np.linalg.inv(Te), 2) for w, Te in zip(W, T))
    err = float(np.linalg.norm(engine.download(dQ, tc.SWEEP_M) - want))
    print("term-operator gmres sweep in batches of 3: err %.3e bound %.3e" % (err, bound))
    assert err <= bound


# ---- 4. callback failure and refusals ------------------------------------------------------------------------------------------------
def test_callback_failure_is_an_error_of_the_call_and_the_handle_stays_usable(engine):
    """A callback that returns 3 and one that raises, each in the middle of a solve: FeastHipError (code 7) naming the callback
    and its term, the exception chained, nothing called afterwards; the same handle then solves."""
    mats, funcs, Z, W, _ = tc.grid_operator()
    X = kc.rand_block(mats[0].shape[0], 5, 4)
    good = tc.term_muls(engine, mats)
    T = tc.dense_t(mats, funcs, Z[tc.FAR_NODE], np.complex128)
    for fail in ("code", "raise"):
        calls = []

        def breaks_on_the_fifth(Y, X_):
            calls.append(1)
            if len(calls) == 5:
                if fail == "raise":
                    raise RuntimeError("the operator broke")
                return 3
            good[2](Y, X_)
        _install(engine, mats, funcs, (Z, W), symmetric=True, muls=[good[0], None, breaks_on_the_fifth])
        engine.set_solver("bicgstab", rtol=1e-12, atol=0.0, maxit=100)
        dX = engine.upload(X)
        with pytest.raises(fk.FeastHipError, match=r"operator callback failed \(which=2, code=%s\)" % ("-1" if fail == "raise" else "3")) as ei:
            engine.nep_solve(tc.FAR_NODE, dX, 5)
        assert ei.value.code == 7 and len(calls) == 5          # nothing was called after the failure
        before = engine.operator_stats()["term_calls"][0]
        assert (isinstance(ei.value.__cause__, RuntimeError) and "the operator broke" in str(ei.value.__cause__)) == (fail == "raise")
        dY, rc = engine.nep_solve(tc.FAR_NODE, dX, 5)          # the same handle solves
        assert rc == 0 and engine.operator_stats()["term_calls"][0] > before
        assert np.linalg.norm(T @ engine.download(dY, 5) - X) <= 1e-10 * np.linalg.norm(X)


def test_refusals_name_the_krylov_solvers_and_leave_the_handle_usable(engine):
    mats, funcs, Z, W, _ = tc.grid_operator()
    N, m = mats[0].shape[0], 5
    X = kc.rand_block(N, m, 4)
    _install(engine, mats, funcs, (Z, W), symmetric=False)
    engine.set_solver("bicgstab", rtol=1e-12, atol=0.0, maxit=200)
    dX = engine.upload(X)
    dXl = engine.upload(kc.rand_block(2 * N, m, 5))          # a linearised block: poly_degree N rows

    def refused(call, *words):
        with pytest.raises(fk.FeastHipError) as ei:
            call()
        assert ei.value.code == 9, ei.value
        for w in SOLVER_NAMES + words:
            assert w in str(ei.value), (w, str(ei.value))

    refused(lambda: engine.set_solver("direct"), "no matrix to factor")
    refused(lambda: engine.set_solver("banded"), "no matrix to factor")
    refused(lambda: engine.set_solver("bicgstab", factor_precision=32), "factor_precision = 32")
    refused(lambda: engine.set_solver("shifted_cocg"), "shifted and block")
    refused(lambda: engine.set_solver("block_cocg"), "shifted and block")
    refused(lambda: engine.set_solver("cocg"), "FEASTHIP_OP_SYMMETRIC")
    refused(lambda: engine.set_adjoint(True), "adjoint")
    refused(lambda: engine.set_node_solver([4] + [0] * (engine.ne - 1)), "direct node")
    refused(lambda: engine.comm_init(1, 0, bytes(128), "shm"), "one rank")
    refused(lambda: engine.set_node_range(0, engine.ne - 1), "whole contour")
    refused(lambda: engine.set_node_list([0, 2]), "whole contour")
    # everything that forms powers of lambda or linearised columns, the count estimate, the pencil entry points
    refused(lambda: engine.poly_solve(Z[0], dX, m), "powers of lambda")
    refused(lambda: engine.poly_eval_cols(dX, np.ones(m), m), "powers of lambda")
    refused(lambda: engine.poly_resinv_apply(dX, m), "powers of lambda")
    refused(lambda: engine.poly_ritz_eval(dX, m, np.eye(m), np.ones(m)), "powers of lambda")
    refused(lambda: engine.poly_contour_apply(dXl, m), "powers of lambda")
    refused(lambda: engine.poly_matmul(0, dXl, m), "powers of lambda")
    refused(lambda: engine.poly_project(dXl, m), "powers of lambda")
    refused(lambda: engine.poly_ritz_residual(dXl, m, np.eye(m), np.ones(m), m), "powers of lambda")
    refused(lambda: engine.poly_estimate_count(m, 1, np.ones((engine.ne, 3))), "count estimate")
    refused(lambda: engine.matmul(0, dX, m), "pencil")
    refused(lambda: engine.shifted_solve(Z[0], dX, m), "pencil")
    refused(lambda: engine.contour_apply(dX, m), "pencil")
    # the backward errors need the norms
    with pytest.raises(fk.FeastHipError, match="feasthip_set_term_norms") as ei:
        engine.nep_ritz_eval(dX, m, np.eye(m), np.ones((m, 3)))
    assert ei.value.code == 9
    # a solver setting left over from a matrix problem becomes one the handle takes
    engine.set_problem(np.eye(N))
    engine.set_solver("direct")
    _install(engine, mats, funcs, (Z, W), symmetric=False)
    # still usable: a solve, a product and, with the norms, the backward errors
    engine.set_solver("gmres", rtol=1e-12, atol=0.0, maxit=300, restart=40)
    dY, rc = engine.nep_solve(tc.FAR_NODE, dX, m)
    assert rc == 0
    T = tc.dense_t(mats, funcs, Z[tc.FAR_NODE], np.complex128)
    assert np.linalg.norm(T @ engine.download(dY, m) - X) <= 1e-9 * np.linalg.norm(X)
    engine.set_term_norms(tc.exact_norms(mats))
    F = nr.table(funcs, np.full(m, 0.5 + 0.1j))
    dXc, be = engine.nep_ritz_eval(dX, m, np.eye(m), F)
    Xn = X / np.linalg.norm(X, axis=0)
    dense = [np.eye(N) if M is None else M for M in mats]
    assert np.allclose(be, nr.candidate_errors(dense, F, Xn), rtol=1e-10)


# ---- 5. drivers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.DRIVER_NAMES)
def test_feast_nonlinear_matvec(engine, name):
    """fk.feast_nonlinear_matvec against the inexact restatement, the closed form and numpy on its vectors
    (test_gpu_nonlinear._check with no factorisation); norms = the exact Frobenius norms, so the measures are the restatement's."""
    mats, funcs, case, _, kw = tc.driver_case(name)
    ref, again = tc.driver_run(name), tc.driver_run(name, 1e-14)
    real = kw["real"]
    terms = list(zip(tc.term_muls(engine, mats, real), funcs))
    Q0 = fo.seeded_subspace(case["N"], case["m0"], tc.DRIVER_SEED)
    res = fk.feast_nonlinear_matvec(terms, case["N"], case["center"], case["radius"], M0=case["m0"], fpm=_fpm(), Q0=Q0,
                                    norms=tc.exact_norms(mats), engine=engine, **kw)
    nep, op = res.stats["nonlinear"], res.stats["operator"]
    print("feast_nonlinear_matvec %s: operator %s krylov %s" % (name, op, [(k["iterations"], k["capped_nodes"]) for k in nep["krylov"]]))
    dense = [np.eye(case["N"]) if M is None else M for M in mats]
    _check(res, ref, again, list(zip(dense, funcs)), case["lam_in"], ne=0)
    assert nep["plan"] == "krylov" and len(nep["krylov"]) == res.loop + 1
    assert all(len(k["node_iterations"]) == tc.NE for k in nep["krylov"])
    assert res.stats["krylov_iterations"] == sum(sum(k["node_iterations"]) for k in nep["krylov"])
    assert op["norms_estimated"] is False and np.allclose(op["norms"], tc.exact_norms(mats))
    assert all((n == 0) == (M is None) for n, M in zip(op["term_calls"], mats)) and op["callback_seconds"] > 0.0


def test_feast_polynomial_matvec_against_the_sparse_polynomial(engine):
    """damped_case("20x16") through its coefficients' products against fk.feast_polynomial on the sparse coefficients under
    method="projected", solver="bicgstab", solver_tol=1e-4: same start block and settings, same info, M and loop, every history
    entry within HISTORY_FACTOR of the other's."""
    columns, seed, _ = ppr.DAMPED_PINS[("20x16", False)]
    case = sc.damped_case("20x16", False)
    Q0 = fo.seeded_subspace(case["N"], columns, seed)
    common = dict(M0=columns, fpm=_fpm(sc.FPM3, sc.NE), Q0=Q0, solver="bicgstab", solver_tol=1e-4, solver_maxiter=2000, engine=engine)
    ref = fk.feast_polynomial(list(case["coeffs"]), case["center"], case["radius"], method="projected", **common)
    dense = sc.dense(case["coeffs"])
    res = fk.feast_polynomial_matvec(tc.term_muls(engine, dense), case["N"], case["center"], case["radius"],
                                     norms=[np.linalg.norm(A) for A in dense], **common)
    a, b = res.stats["polynomial"], ref.stats["polynomial"]
    print("feast_polynomial_matvec: loop %d (sparse %d) history %s (sparse %s) operator %s" % (
        res.loop, ref.loop, ["%.2e" % e for e in a["eps_history"]], ["%.2e" % e for e in b["eps_history"]], res.stats["operator"]))
    assert ref.info == 0 and res.info == ref.info and res.M == ref.M == case["k"] and res.loop == ref.loop
    assert len(a["eps_history"]) == len(b["eps_history"])
    for x, y in zip(a["eps_history"], b["eps_history"]):
        assert y / pkr.HISTORY_FACTOR <= x <= y * pkr.HISTORY_FACTOR, (a["eps_history"], b["eps_history"])
    assert a["plan"] == "krylov" and a["degree"] == 2 and a["method"] == "projected" and a["columns"] == columns
    assert "nonlinear" not in res.stats and res.stats["factorizations"] == 0 and len(a["krylov"]) == res.loop + 1


def test_norms_are_estimated_when_none_are_given(engine):
    """norms=None on the grid delay operator (N = 120): 32 seeded +-1 columns give ||A_k||_F within 30 % -- the estimator's
    relative standard deviation is at most sqrt(2 / 32) = 25 % even for a rank-one matrix, and these are far from that --
    sqrt(N) exactly for the identity, one call per non-identity term; the run converges on the estimated measure."""
    mats, funcs, case, _, kw = tc.driver_case("grid-6x5x4-cocg")
    res = fk.feast_nonlinear_matvec(list(zip(tc.term_muls(engine, mats), funcs)), case["N"], case["center"], case["radius"],
                                    M0=case["m0"], fpm=_fpm(), seed=tc.DRIVER_SEED, engine=engine, **kw)
    op = res.stats["operator"]
    ratio = np.array(op["norms"]) / np.array(tc.exact_norms(mats))
    print("estimated norms / exact: %s" % ratio)
    assert res.info == 0 and res.M == case["count"] and op["norms_estimated"] is True
    assert nr.match_error(res.lambda_, case["lam_in"]) <= 1e-8
    assert np.all(np.abs(ratio - 1.0) <= 0.3) and op["norms"][1] == np.sqrt(case["N"])
