"""Block COCG sweep (FEASTHIP_SOLVER_BLOCK_COCG) on the device: against its step-exact restatement
(block_cocg_reference.py; inputs in block_cocg_cases.py), bitwise reproducibility, the breakdown fallback, the ineligible
paths and a FEAST solve end to end.

Error model of test_gpu_krylov_steps.py: the device block must lie within br.tolerance(D) = max(32 D, 64 eps) of the
long-double restatement, D the restatement's own complex128 drift over br.DRIFT_ORDERS (asserted below 1e-6 / 32 on the host)."""
import numpy as np
import pytest
import scipy.sparse as sp

import krylov_reference as kr
import block_cocg_reference as br
import block_cocg_cases as bc

pytestmark = pytest.mark.gpu
fk = bc.fk


@pytest.fixture(autouse=True)
def restore(engine):
    yield
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.set_column_mask(None)
    engine.set_node_solver(None)


def run(engine, c, solver="block_cocg", **kw):
    engine.set_problem(c.A, c.B)
    engine.set_contour(c.Zall, c.Wall, c.scale)
    engine.set_node_list(c.nodes)
    engine.set_real_projection(False)
    engine.set_node_solver(None)
    engine.set_solver(solver, rtol=c.rtol, atol=0.0, maxit=c.maxit, **kw)
    engine.set_column_mask(c.mask)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), c.m, c.ritz)
    return engine.download(dP, c.m), list(status)[:len(c.nodes)], st


def test_solver_kind_and_query_exist(engine):
    """Fails without the feature: kind 6 is FEASTHIP_ERROR_FPM and feasthip_last_block_sweep is not exported."""
    assert engine.lib.feasthip_set_solver(engine.h, 6, 1e-3, 0.0, 50, 30, 64, 1) == 0
    assert hasattr(engine.lib, "feasthip_last_block_sweep")
    engine.set_solver("block_cocg", rtol=1e-3, maxit=10)


@pytest.mark.parametrize("cid", [k for k in bc.CASES if not k.endswith("breakdown")])
def test_sweep_is_the_restatement_step_for_step(engine, cid):
    c = bc.case(cid)
    try:
        out, status, st = run(engine, c)
        used, steps_max, brk, passes = engine.last_block_sweep()
        dist = kr.block_dist(out, c.ref.out)
        print("block-steps %s D=%.3e device=%.3e tol=%.3e" % (cid, c.drift, dist, br.tolerance(c.drift)))
        assert used and brk == 0 == c.ref.breakdowns
        assert list(engine.last_node_iterations(len(c.nodes))) == list(c.ref.steps)
        assert steps_max == c.ref.steps_max and passes == c.ref.passes
        assert status == list(c.ref.status)
        counts = np.asarray(engine.last_column_iterations(len(c.nodes), c.m))
        assert np.array_equal(counts, np.array([nd.iters for nd in c.ref.nodes]))
        assert dist <= br.tolerance(c.drift), (cid, dist, c.drift)
        out2, status2, _ = run(engine, c)
        assert out2.tobytes() == out.tobytes() and status2 == status
        assert engine.last_block_sweep() == (used, steps_max, brk, passes)
    finally:
        engine.set_node_list(np.arange(16))


def test_breakdown_finishes_through_the_per_column_sweep(engine):
    c = bc.case("lap/1/m5/breakdown")
    try:
        out, status, st = run(engine, c)
        used, steps_max, brk, passes = engine.last_block_sweep()
        assert used and brk == 1 and steps_max == 0
        assert status == [0]                                        # every column converged in the fallback
        dist = kr.block_dist(out, c.ref.out)
        print("block-breakdown D=%.3e device=%.3e" % (c.drift, dist))
        assert dist <= br.tolerance(c.drift)
    finally:
        engine.set_node_list(np.arange(16))


@pytest.mark.parametrize("path", ["complex-A", "dense", "factor-precision-32"])
def test_ineligible_call_is_the_cocg_sweep_bit_for_bit(engine, path):
    A, B, _ = bc.problem("lap")
    N = A.shape[0]
    if path == "complex-A":
        A = sp.csr_matrix(A.astype(np.complex128))
    if path == "dense":
        A, B = fk.workloads.laplacian_3d_pencil(6, 5, 4)[:2]
        A, B, N = A.toarray(), B.toarray(), A.shape[0]
    Z, W = bc.contour("lap", 40)
    Q = np.array(fk.seeded_subspace(N, 9))
    got = {}
    for solver in ("cocg", "block_cocg"):
        engine.set_problem(A, B); engine.set_contour(Z, W, 2.0); engine.set_real_projection(True)
        engine.set_node_list(np.arange(16)); engine.set_node_solver(None)
        engine.set_solver(solver, rtol=3e-2, atol=0.0, maxit=40, factor_precision=32 if path == "factor-precision-32" else 64)
        try:
            r = engine.contour_apply(engine.upload(Q), 9, None)
            got[solver] = ("ok", engine.download(r[0], 9), list(r[1]), engine.last_column_iterations(16, 9).copy())
        except fk.FeastHipError as e:
            got[solver] = ("error", str(e))
        assert engine.last_block_sweep()[0] is False
    a, b = got["cocg"], got["block_cocg"]
    assert a[0] == b[0]
    if a[0] == "ok":
        assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and np.array_equal(a[3], b[3])
    else:
        assert a[1] == b[1]


def test_feast_end_to_end():
    A, B, lam = fk.workloads.laplacian_3d_pencil(20, 16, 10)[:3]
    interval = (0.0, 0.42)
    inside = np.sort(lam[(lam >= interval[0]) & (lam <= interval[1])])
    assert 4 <= len(inside) <= 48
    res = {}
    for solver in ("cocg", "block_cocg"):
        fpm = fk.feastinit()
        fpm[2] = 16
        res[solver] = fk.feast(A, B, interval, M0=int(1.5 * len(inside)) + 8, fpm=fpm, solver=solver, warm_start=True,
                               inner_rtol=3e-2, solver_maxiter=50)
    r, r0 = res["block_cocg"], res["cocg"]
    print("block-feast loops: block %d, cocg %d; epsout %.2e / %.2e; block stats %s" % (r.loop, r0.loop, r.epsout, r0.epsout, r.stats["block"]))
    assert r.info == 0 and r.M == len(inside)
    assert np.abs(np.sort(r.lambda_) - inside).max() <= 1e-10
    X, l = np.asarray(r.q)[:, :r.M], np.asarray(r.lambda_)[:r.M]
    R = A @ X - (B @ X) * l[None, :]
    rel = np.linalg.norm(R, axis=0) / (np.linalg.norm(X, axis=0) * max(abs(interval[0]), abs(interval[1])))
    assert rel.max() <= 1e-12, rel.max()
    assert r.loop <= r0.loop + 1
    assert len(r.stats["block"]) >= r.loop and all(s["used"] for s in r.stats["block"])
    assert "block" not in r0.stats
