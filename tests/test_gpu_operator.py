"""Operator handles (feasthip_set_operator, engine.set_operator, csrc/fh_operator.hip) on the device: matrix-free FEAST on the
caller's products.  Inputs and references: operator_cases.py; the conditions on the references alone: test_operator_host.py.

Products are compared with the long-double product within 16 N eps ||M||_F ||X||_F; truncated solves and sweeps with the
step-exact restatements (krylov_reference.py, gmres_reference.py) within krylov_reference.tolerance(D), D measured at test
time, on the same pencils the dense handle is held to.  The callbacks multiply by the same dense A and B with torch.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import gmres_cases as gc
import krylov_cases as kc
import krylov_reference as kr
import operator_cases as oc
from test_gpu_gmres_steps import check_sweep as gmres_check_sweep
from test_gpu_krylov_steps import check_sweep as krylov_check_sweep, close_enough

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KRYLOV_NAMED = "FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES"


@pytest.fixture(autouse=True)
def restore(engine, monkeypatch):
    monkeypatch.delenv("FH_GMRES_BUDGET_MB", raising=False)
    yield
    engine.set_problem(np.eye(4))               # an ordinary handle again: the other files' fixtures set the direct solver
    engine.set_node_solver(None)
    engine.set_column_mask(None)
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.set_column_block(0, -1)


def product_error(Y, M, X):
    """(Frobenius distance to the long-double product, the bound 16 N eps ||M||_F ||X||_F)"""
    ref = M.astype(np.clongdouble) @ X.astype(np.clongdouble)
    return float(np.linalg.norm(Y.astype(np.clongdouble) - ref)), 16.0 * M.shape[0] * EPS * np.linalg.norm(M) * np.linalg.norm(X)


# ---- 1. products -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real-view", "complex"])
@pytest.mark.parametrize("m", [7, 24, 40, 72])
def test_products(engine, m, cplx):
    """engine.matmul(0 | 1) at N = 63 (a multiple of no tile) for ld = 16, 32, 64 and two panels.  (m = 72 runs at N = 95: every
    entry point requires m <= N.)  The host hint keeps the other operator's callback from being made."""
    N = 63 if m <= 63 else 95
    A, B, X = oc.product_inputs(N, m, cplx)
    oc.set_matrix_operator(engine, A, B, real=not cplx)
    dX = engine.upload(X)
    panels = (m + 63) // 64
    for which, M in ((0, A), (1, B)):
        before = engine.operator_stats()
        Y = engine.download(engine.matmul(which, dX, m), m)
        after = engine.operator_stats()
        err, bound = product_error(Y, M, X)
        print("operator product N=%d m=%d which=%d %s: error %.3e bound %.3e" % (N, m, which, "complex" if cplx else "real", err, bound))
        assert err <= bound
        mine, other = ("A_calls", "B_calls") if which == 0 else ("B_calls", "A_calls")
        assert after[mine] - before[mine] == panels and after[other] == before[other]


@pytest.mark.parametrize("cplx", [False, True], ids=["real-view", "complex"])
def test_product_where_the_combine_loop_takes_a_second_trip(engine, cplx):
    """N = 6007, m = 40 (ld = 64): N ld = 384 448 elements against the grid limit of 1024 workgroups x 256 threads = 262 144
    (fh_op_combine_nblk), so half of the workgroups take a second trip of the grid-stride loop.  A matrix-free banded
    operator; B = I returns X itself."""
    N, m = 6007, 40
    mul, host, fro = oc.band_mul(engine, N, cplx)
    X = kc.rand_block(N, m, 3)
    engine.set_operator(N, mul, None, real=not cplx)
    dX = engine.upload(X)
    Y = engine.download(engine.matmul(0, dX, m), m)
    err = float(np.linalg.norm(Y.astype(np.clongdouble) - host(X)))
    bound = 16.0 * N * EPS * fro * np.linalg.norm(X)
    print("operator product N=%d m=%d: error %.3e bound %.3e" % (N, m, err, bound))
    assert err <= bound
    before = engine.operator_stats()
    assert np.array_equal(engine.download(engine.matmul(1, dX, m), m), X)
    assert engine.operator_stats()["A_calls"] == before["A_calls"] and engine.operator_stats()["B_calls"] == 0


# ---- 2. truncated solves are the k-th iterate --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("mod,name,solver", oc.TRUNC, ids=[t[1] for t in oc.TRUNC])
def test_truncated_solve_is_the_kth_iterate(engine, mod, name, solver, near):
    """The cases of test_gpu_krylov_steps.py / test_gpu_gmres_steps.py on their dense pencils, through an operator handle whose
    callbacks multiply by the same A and B: the iterate within tolerance(D), return code, step counts, and for GMRES the
    products (cycle starts plus the lock-steps that ran)."""
    c = oc.trunc_case(mod, name, near)
    oc.set_matrix_operator(engine, c.A, c.B, real=True, symmetric=True)
    dX = engine.upload(c.X)
    assert len(c.columns) == c.m and c.m <= 64
    for k in c.ks:
        kw = {"restart": c.restart} if solver == "gmres" else {}
        engine.set_solver(solver, rtol=1e-14, atol=0.0, maxit=k, **kw)
        dY, rc = engine.shifted_solve(c.z, dX, c.m)
        Y = engine.download(dY)
        st = engine.last_stats
        want = c.want[k] if solver == "gmres" else [kr.truncated(r, k) for r in c.ref]      # (x, steps, status, active, margin)
        decided = [w[4] >= kc.MARGIN_MIN for w in want]
        assert sum(not d for d in decided) <= kc.LEFT_OUT_MAX * len(want)
        if all(decided):
            assert rc == (kr.NO_CONVERGENCE if any(w[3] for w in want) else 0), (name, k, rc)
            if solver == "gmres":
                if any(w[1] == k for w in want):
                    assert st["krylov_iterations"] == k, (name, k, st)
                    assert st["spmm_calls"] == c.products[k], (name, k, st, c.products[k])
            else:
                assert st["krylov_iterations"] == (k if any(w[3] for w in want) else max(w[1] for w in want)), (name, k, st)
        dist = max(kr.rel_dist(Y[:, j], w[0]) for j, w, ok in zip(c.columns, want, decided) if ok)
        close_enough("operator/truncated/%s/%s/k=%d" % (name, "near" if near else "far", k), dist, c.drift[k])


# ---- 3. sweeps with mixed stops ----------------------------------------------------------------------------------------------------------
def setup_sweep(engine, c, symmetric, batched=False, seen=None):
    A, B = oc.dense_of(c.A), oc.dense_of(c.B)
    if seen is None:
        oc.set_matrix_operator(engine, A, B, real=True, symmetric=symmetric, batched=batched)
    else:
        a, b = oc.over_nodes(oc.matrix_mul(engine, A)), oc.over_nodes(oc.matrix_mul(engine, B))

        def a_seen(Y, X):
            seen.append(X.shape[0])
            a(Y, X)
        engine.set_operator(A.shape[0], a_seen, b, real=True, symmetric=symmetric, batched=True)
    engine.set_contour(c.Z, c.W, c.scale)
    engine.set_real_projection(True)
    engine.set_column_block(0, -1)
    engine.set_node_solver(None)
    engine.set_column_mask(None)


@pytest.mark.parametrize("method,solver,rtol,maxit,warm", oc.SWEEPS,
                         ids=["%s-maxit%d-%s" % (s[1], s[3], "ritz" if s[4] else "zero") for s in oc.SWEEPS])
def test_krylov_sweep_with_mixed_stops(engine, method, solver, rtol, maxit, warm):
    """8 nodes, m = 24: nodes and columns leave at different steps (node_active, the per-node partial rows of
    k_op_combine), at maxit = 7 the cap bites.  The summed block, per-node status, per-column steps over the decided pairs and
    the node counts equal the restatement's on the same pencil; the resident entry point gives the same."""
    c = oc.sweep_case(method, rtol, maxit, warm)
    setup_sweep(engine, c, True)
    engine.set_solver(solver, rtol=rtol, atol=0.0, maxit=maxit)
    n, m = len(c.Z), c.m
    dQ = engine.upload(c.Q)
    tag = "operator/sweep/%s/maxit=%d/%s" % (solver, maxit, "ritz" if warm else "zero")
    dP, status, st = engine.contour_apply(dQ, m, c.ritz)
    krylov_check_sweep(tag, c, engine.download(dP, m), status, True, engine.last_column_iterations(n, m),
                       engine.last_node_iterations(n), st)
    status2, st2 = engine.contour_apply_resident(dQ, m, c.ritz)
    krylov_check_sweep(tag + "/resident", c, engine.download(engine.export_resident(m, which=1), m), status2, True,
                       engine.last_column_iterations(n, m), engine.last_node_iterations(n), st2)


def test_gmres_sweep_in_node_batches_of_three(engine, monkeypatch):
    """The 8-node GMRES sweep under FH_GMRES_BUDGET_MB batches of 3: the callback sees nodes = 3, 3 and 2 (and 1 for the
    right-hand side B Q); iterates, steps, statuses and products equal the batch-level restatement's."""
    kind, m, warm, setting = oc.GMRES_SWEEP
    rtol, maxit, restart = setting
    c = oc.gmres_sweep_case()
    seen = []
    setup_sweep(engine, c, False, seen=seen)
    engine.set_solver("gmres", rtol=rtol, atol=0.0, maxit=maxit, restart=restart)
    monkeypatch.setenv("FH_GMRES_BUDGET_MB", str(gc.budget_mb(c.A.shape[0], m, restart, oc.GMRES_BATCH)))
    n = len(c.Z)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), m, c.ritz)
    assert set(seen) >= {3, 2} and 8 not in seen, seen
    gmres_check_sweep("operator/sweep/gmres/batch=3", c, True, engine.download(dP, m), status, st,
                      engine.last_column_iterations(n, m), engine.last_node_iterations(n))


# ---- 4. callback failure -----------------------------------------------------------------------------------------------------------------
def test_callback_failure_is_an_error_of_the_call_and_the_handle_stays_usable(engine):
    """A callback that returns 3 and one that raises: FeastHipError (code 7) naming the operator callback, the exception
    chained; a failure in the middle of a Krylov solve likewise; the next product on the same engine is right."""
    N, m = 63, 7
    A, B, X = oc.solve_pair(N, m)
    good = oc.matrix_mul(engine, A)
    dX = engine.upload(X)
    engine.set_operator(N, lambda Y, X_: 3, None)
    with pytest.raises(fk.FeastHipError, match=r"operator callback failed \(which=0, code=3\)") as ei:
        engine.matmul(0, dX, m)
    assert ei.value.code == 7

    def boom(Y, X_):
        raise RuntimeError("the operator broke")
    engine.set_operator(N, good, boom)
    with pytest.raises(fk.FeastHipError, match=r"operator callback failed \(which=1") as ei:
        engine.matmul(1, dX, m)
    assert ei.value.code == 7 and isinstance(ei.value.__cause__, RuntimeError) and "the operator broke" in str(ei.value.__cause__)
    err, bound = product_error(engine.download(engine.matmul(0, dX, m), m), A, X)
    assert err <= bound

    calls = []

    def fails_on_the_fifth(Y, X_):
        calls.append(1)
        if len(calls) == 5:
            raise RuntimeError("fifth call")
        good(Y, X_)
    engine.set_operator(N, fails_on_the_fifth, None)
    engine.set_solver("bicgstab", rtol=1e-12, atol=0.0, maxit=50)
    with pytest.raises(fk.FeastHipError, match="operator callback failed") as ei:
        engine.shifted_solve(-3.0 + 2.0j, dX, m)
    assert isinstance(ei.value.__cause__, RuntimeError) and len(calls) == 5          # nothing was called after the failure
    dY, rc = engine.shifted_solve(-3.0 + 2.0j, dX, m)                                  # the same handle solves
    assert rc == 0
    Y = engine.download(dY, m)
    S = (-3.0 + 2.0j) * np.eye(N) - A
    assert np.linalg.norm(S @ Y - X) <= 1e-10 * np.linalg.norm(X)
    err, bound = product_error(engine.download(engine.matmul(0, dX, m), m), A, X)
    assert err <= bound


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_krylov_solvers_and_leave_the_handle_usable(engine):
    N, m = 63, 7
    A, B, X = oc.solve_pair(N, m)
    oc.set_matrix_operator(engine, A, B, real=True, symmetric=False)
    engine.set_contour(*kc.contour8(0.0, 1.0), 2.0)
    engine.set_solver("bicgstab", rtol=1e-12, atol=0.0, maxit=100)
    engine.poly_degree = 1                       # (what the engine's poly_* / nep_* wrappers size their blocks by)
    dX = engine.upload(X)

    def refused(call, *words):
        with pytest.raises(fk.FeastHipError) as ei:
            call()
        assert ei.value.code == 9, ei.value
        for w in (KRYLOV_NAMED,) + words:
            assert w in str(ei.value), (w, str(ei.value))

    refused(lambda: engine.set_solver("direct"), "no matrix to factor")
    refused(lambda: engine.set_solver("banded"), "no matrix to factor")
    refused(lambda: engine.set_solver("cocg"), "FEASTHIP_OP_SYMMETRIC")
    refused(lambda: engine.set_solver("shifted_cocg"), "FEASTHIP_OP_SYMMETRIC")
    refused(lambda: engine.set_solver("bicgstab", factor_precision=32), "factor_precision = 32")
    refused(lambda: engine.set_adjoint(True), "adjoint")
    refused(lambda: engine.set_node_solver([4] + [0] * (engine.ne - 1)), "direct node")
    refused(lambda: engine.comm_init(1, 0, bytes(128), "shm"), "communicator")
    refused(lambda: engine.poly_matmul(0, dX, m), "feasthip_set_operator")
    refused(lambda: engine.poly_orthonormalize(dX, m, 1e-8), "feasthip_set_operator")
    refused(lambda: engine.nep_eval_cols(dX, np.ones((m, 2)), m), "feasthip_set_operator")
    # a solver setting left over from a matrix problem is refused when the solve is asked for
    engine.set_problem(np.eye(N))
    engine.set_solver("direct")
    oc.set_matrix_operator(engine, A, B, real=True, symmetric=False)
    refused(lambda: engine.shifted_solve(0.3 + 1.0j, dX, m), "no matrix to factor")
    refused(lambda: engine.contour_apply(dX, m), "no matrix to factor")
    # still usable: the solver it takes, a solve and a product
    engine.set_solver("gmres", rtol=1e-12, atol=0.0, maxit=200, restart=30)
    z = 0.3 + 1.0j
    dY, rc = engine.shifted_solve(z, dX, m)
    assert rc == 0
    Y = engine.download(dY, m)
    assert np.linalg.norm((z * B - A) @ Y - X) <= 1e-9 * np.linalg.norm(X)
    err, bound = product_error(engine.download(engine.matmul(1, dX, m), m), B, X)
    assert err <= bound


# ---- 6. drivers --------------------------------------------------------------------------------------------------------------------------
LAPLACE_INTERVAL = (0.0, 1.0)


def test_feast_matvec_on_the_slicing_laplacian(engine):
    """B = I, symmetric, COCG: the count, the closed-form eigenvalues and host residuals with the scipy matrix."""
    lam = oc.laplacian_eigenvalues()
    Emin, Emax = LAPLACE_INTERVAL
    inside = lam[(lam >= Emin) & (lam <= Emax)]
    assert 4 <= len(inside) <= 24
    fpm = fk.feastinit()
    res = fk.feast_matvec(oc.laplacian_mul(), None, len(lam), (Emin, Emax), M0=32, fpm=fpm, solver="cocg", symmetric=True,
                          engine=engine)
    print("feast_matvec laplacian: info %d M %d loops %d epsout %.2e operator %s" % (res.info, res.M, res.loop, res.epsout, res.stats["operator"]))
    assert res.info == 0 and res.M == len(inside)
    order = np.argsort(res.lambda_)
    assert np.abs(res.lambda_[order] - inside).max() <= 1e-10
    L = oc.laplacian_matrix()
    q = res.q[:, order]
    r = np.linalg.norm(L @ q - q * res.lambda_[order], axis=0) / (np.linalg.norm(q, axis=0) * max(abs(Emin), abs(Emax)))
    assert r.max() <= 10.0 * 10.0 ** (-int(fpm[3])), r
    op = res.stats["operator"]
    assert op["A_calls"] > 0 and op["B_calls"] == 0 and op["callback_seconds"] > 0.0


def test_feast_matvec_with_a_diagonal_b_and_the_default_gmres(engine):
    """The same operator with a diagonal B under the defaults (GMRES(20), 1e-6, 200) against fk.feast on the CSR matrices."""
    L = oc.laplacian_matrix()
    N = L.shape[0]
    d = oc.diagonal_b(N)
    Bm = sp.diags(d).tocsr()
    Emin, Emax = 0.0, 0.6
    ref = fk.feast(L, Bm, (Emin, Emax), M0=32, solver="gmres", solver_tol=1e-6, solver_maxiter=200, solver_restart=20,
                   warm_start=True, engine=engine)                       # (feast_matvec's defaults, spelled out)
    res = fk.feast_matvec(oc.laplacian_mul(), oc.diagonal_mul(engine, d), N, (Emin, Emax), M0=32, engine=engine)
    print("feast_matvec diag B: info %d M %d loops %d (matrix: info %d M %d loops %d) operator %s"
          % (res.info, res.M, res.loop, ref.info, ref.M, ref.loop, res.stats["operator"]))
    assert ref.info == 0 and res.info == 0 and res.M == ref.M > 0
    assert np.abs(np.sort(res.lambda_) - np.sort(ref.lambda_)).max() <= 1e-10
    assert res.stats["operator"]["B_calls"] > 0


def test_feast_general_matvec_on_convection_diffusion(engine):
    """A real, non-symmetric operator under BiCGStab against fk.feast_general on the dense matrix with the direct solver.  The
    inner solves stop at 1e-9 (BiCGStab's recursive residual does not reach 1e-12 next to the spectrum in 500 steps); the
    refinement loops take the Ritz residuals to 10^-fpm[3] all the same."""
    C = oc.convection_diffusion()
    N = C.shape[0]
    center, radius = 0.6 + 0.0j, 0.4
    ref = fk.feast_general(C, None, center, radius, M0=24, engine=engine)
    res = fk.feast_general_matvec(oc.matrix_mul(engine, C), None, N, center, radius, M0=24, solver="bicgstab", solver_tol=1e-9,
                                  solver_maxiter=1000, engine=engine)
    print("feast_general_matvec: info %d M %d loops %d (matrix: info %d M %d)" % (res.info, res.M, res.loop, ref.info, ref.M))
    assert ref.info == 0 and res.info == 0 and res.M == ref.M > 0
    a, b = np.sort_complex(np.asarray(res.lambda_)), np.sort_complex(np.asarray(ref.lambda_))
    assert np.abs(a - b).max() <= 1e-8
    # and a complex operator through complex128 panels, under GMRES(100)
    Cc = C + 0.05j * np.diag(np.arange(N) / N)
    refc = fk.feast_general(Cc, None, center, radius, M0=24, engine=engine)
    resc = fk.feast_general_matvec(oc.matrix_mul(engine, Cc, real=False), None, N, center, radius, M0=24, solver="gmres",
                                   solver_tol=1e-9, solver_maxiter=1000, solver_restart=100, real=False, engine=engine)
    assert refc.info == 0 and resc.info == 0 and resc.M == refc.M > 0
    assert np.abs(np.sort_complex(np.asarray(resc.lambda_)) - np.sort_complex(np.asarray(refc.lambda_))).max() <= 1e-8


def test_the_hermitian_probe_rejects_a_nonsymmetric_operator(engine):
    C = oc.convection_diffusion()
    with pytest.raises(ValueError, match="A is not Hermitian"):
        fk.feast_matvec(oc.matrix_mul(engine, C), None, C.shape[0], (0.1, 1.1), M0=24, solver="bicgstab", engine=engine)
    L = oc.laplacian_matrix()
    with pytest.raises(ValueError, match="B is not Hermitian"):
        fk.feast_matvec(oc.laplacian_mul(), oc.matrix_mul(engine, np.eye(L.shape[0]) + 0.01 * np.triu(np.ones(L.shape), 1)),
                        L.shape[0], (0.0, 0.6), M0=24, solver="bicgstab", engine=engine)
