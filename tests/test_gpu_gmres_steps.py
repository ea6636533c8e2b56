"""Device GMRES(m) (csrc/fh_gmres.hip, fh_gmres in csrc/fh_api.hip) against the step-exact batch-level restatement
(gmres_reference.py; inputs and reference results in gmres_cases.py).

Every case compares the returned block with the long-double reference iterate / sweep, the per-column step counts, the
node statuses and return codes, and feasthip_stats.spmm_calls with the reference's product count (one per cycle start and
one per lock-step that RAN: the check that a step queued behind the last live column of a cycle is not counted).  The
tolerance is measured at test time exactly as in test_gpu_krylov_steps.py: D = the drift of the restatement itself in
complex128 over four summation orders against long double, and the device must lie within max(32 D, 64 eps)
(krylov_reference.tolerance); 32 D <= 1e-7 is asserted for every compared case.  (node, column) pairs whose stop is
decided by less than 1e-6 are left out, at most 2 % of a case (asserted); the reference leaves out none.

Measured on an MI355X (83 cases, all pass, none skipped, no pair left out); per group the number of comparisons, the
largest D, the largest distance of the device from the long-double reference and the largest share of its tolerance
(at least 64 eps = 1.4e-14) that the device used:

    truncated, far shift        51   D <= 1.9e-15   device <= 1.9e-15   0.03
    truncated, near shift       51   D <= 1.2e-13   device <= 4.8e-14   0.03
    own stop step, per column  138   D <= 5.9e-16   device <= 2.0e-15   0.11
    exhaustion                   2   D <= 9.3e-16   device <= 8.3e-16   0.04
    sweeps, batches 8 / 3 / 1   48   D <= 1.4e-14   device <= 7.5e-15   0.03
    mask                         1   D <= 5.4e-15   device <= 4.8e-15   0.03
"""
import os

import numpy as np
import pytest

import gmres_cases as gc
import krylov_reference as kr

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("FH_KRYLOV_STEPS_REPORT")        # measurement runs: the file of test_gpu_krylov_steps.py


def close_enough(group, dist, D):
    print("gmres-steps %s D=%.3e device=%.3e tol=%.3e" % (group, D, dist, kr.tolerance(D)))
    if REPORT:
        with open(REPORT, "a") as f:
            f.write("gmres/%s %.3e %.3e\n" % (group, D, dist))
    assert 32.0 * D <= gc.POWER, (group, D)              # a condition on the reference alone
    assert dist <= kr.tolerance(D), (group, dist, D)


def use_gmres(engine, rtol, atol, maxit, restart):
    engine.set_node_solver(None)
    engine.set_column_mask(None)
    engine.set_solver("gmres", rtol=rtol, atol=atol, maxit=maxit, restart=restart)


@pytest.fixture(autouse=True)
def restore(engine, monkeypatch):
    monkeypatch.delenv("FH_GMRES_BUDGET_MB", raising=False)
    yield
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.set_column_block(0, -1)
    engine.set_column_mask(None)


# ---- truncated single-shift solves: the iteration cap inside a cycle, on a cycle boundary, one step after it -----------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("name", list(gc.TRUNC))
def test_truncated_solve_is_the_kth_iterate(engine, name, near):
    """maxit = k, rtol = 1e-14: rc 5, Y is the reference's iterate after k lock-steps (the cycle cut at ksteps < mr, or ended
    exactly at the cap), k iterations per 64-column panel, and the products are the cycle starts plus the k steps."""
    c = gc.trunc_case(name, near)
    engine.set_problem(c.A, c.B)
    dX = engine.upload(c.X)
    npanels = (c.m + 63) // 64
    for k in c.ks:
        use_gmres(engine, gc.RTOL_TRUNC, 0.0, k, c.restart)
        dY, rc = engine.shifted_solve(c.z, dX, c.m)
        Y = engine.download(dY)
        st = engine.last_stats
        want = c.want[k]                                 # (x, steps, status, active, margin) per compared column
        decided = [w[4] >= gc.MARGIN_MIN for w in want]
        assert sum(not d for d in decided) <= gc.LEFT_OUT_MAX * len(want)
        if all(decided):
            by_panel = [[w for j, w in zip(c.columns, want) if j // 64 == p] for p in range(npanels)]
            if any(w[3] for w in want):
                assert rc == kr.NO_CONVERGENCE, (name, k, rc)
            elif len(c.columns) == c.m:
                assert rc == 0, (name, k, rc)
            if all(any(w[1] == k for w in p) for p in by_panel):
                # a column of every panel took all k lock-steps: the panel's count is k whatever the others did
                assert st["krylov_iterations"] == k * npanels, (name, k, st)
                assert st["spmm_calls"] == c.products[k] * npanels, (name, k, st, c.products[k])
        dist = max(kr.rel_dist(Y[:, j], w[0]) for j, w, ok in zip(c.columns, want, decided) if ok)
        close_enough("truncated/%s/%s/k=%d" % (name, "near" if near else "far", k), dist, c.drift[k])


# ---- sweeps -----------------------------------------------------------------------------------------------------------
def setup_sweep(engine, c, real):
    engine.set_problem(c.A, c.B)
    engine.set_contour(c.Z, c.W, c.scale)
    engine.set_real_projection(real)
    engine.set_column_block(0, -1)


def run_sweep(engine, c):
    n = len(c.Z)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), c.m, c.ritz)
    return engine.download(dP, c.m), status, st, engine.last_column_iterations(n, c.m), engine.last_node_iterations(n)


def check_sweep(group, c, real, out, status, st, counts, node_its):
    """Columns with an undecidable pair are left out (at most 2 % of the pairs)."""
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= gc.LEFT_OUT_MAX * c.decided.size
    ok = np.flatnonzero(c.col_ok)
    cols = [c.columns[i] for i in ok]
    ref = gc.project(c.ref.out, real)[:, ok]
    close_enough(group, kr.block_dist(out[:, cols], ref), c.drift[real])
    dev = np.asarray(counts)[:, c.columns]
    assert np.array_equal(dev[c.decided], c.ref.steps[c.decided]), (group, dev, c.ref.steps)
    if c.decided.all() and len(c.columns) == c.m:
        rowmax = c.ref.steps.max(axis=1)
        assert list(status[:len(c.Z)]) == list(c.ref.status), (group, status, c.ref.status)
        assert list(node_its) == list(rowmax), (group, node_its, rowmax)
        assert st["krylov_iterations"] == rowmax.sum(), (group, st, rowmax)
        assert st["spmm_calls"] == c.ref.products, (group, st, c.ref.products, c.ref.lock_steps)


@pytest.mark.parametrize("restart", gc.STOP_RESTARTS)
@pytest.mark.parametrize("rtol,atol", gc.STOP_SETTINGS)
def test_every_column_stops_at_its_own_step(engine, rtol, atol, restart):
    """Columns that leave at different steps of one cycle (active, inv = 0 and kdim per column), the zero column, the
    column below atol, the pad columns of LD = 16: per-column iters, the node status and each column's iterate."""
    c = gc.stop_case(rtol, atol, restart)
    assert len(set(c.ref.steps[0])) >= 6
    setup_sweep(engine, c, False)
    use_gmres(engine, rtol, atol, 400, restart)
    out, status, st, counts, node_its = run_sweep(engine, c)
    assert not out[:, 5].any() and counts[0, 5] == 0
    if atol > 0:
        assert not out[:, 11].any() and counts[0, 11] == 0
    check_sweep("stops/rtol=%g/atol=%g/restart=%d" % (rtol, atol, restart), c, False, out, status, st, counts, node_its)
    for j in np.flatnonzero(c.col_ok):
        if c.ref.steps[0, j]:
            close_enough("stops/rtol=%g/atol=%g/restart=%d/col=%d/step=%d" % (rtol, atol, restart, j, c.ref.steps[0, j]),
                         kr.rel_dist(out[:, j], c.ref.out[:, j]), c.drift[False])


@pytest.mark.parametrize("name", list(gc.EXHAUST))
def test_krylov_space_exhaustion(engine, name):
    """N <= restart and a right-hand side in a 5-dimensional invariant subspace: h_{k+1,k} is round-off, not 0.0; the
    column leaves on the estimate at the step that exhausts the space, status 0, with the reference's iterate."""
    c = gc.exhaust_case(name)
    assert (c.ref.steps == c.dim).all() and c.decided.all()
    setup_sweep(engine, c, False)
    use_gmres(engine, 1e-10, 0.0, 400, 30)
    out, status, st, counts, node_its = run_sweep(engine, c)
    check_sweep("exhaustion/" + name, c, False, out, status, st, counts, node_its)


def set_batch(monkeypatch, c, restart, batch):
    if batch != len(c.Z):
        monkeypatch.setenv("FH_GMRES_BUDGET_MB", str(gc.budget_mb(c.A.shape[0], c.m, restart, batch)))


@pytest.mark.parametrize("batch", gc.BATCHES)
@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("case", range(len(gc.SWEEPS)), ids=["%s-m%d-%s-rtol%g" % (s[0], s[1], "ritz" if s[2] else "zero", s[3][0])
                                                            for s in gc.SWEEPS])
def test_gmres_sweep(engine, monkeypatch, case, real, batch):
    """8-node sweeps through feasthip_contour_apply under node batches of 8, 3 and 1 (FH_GMRES_BUDGET_MB: the e0 offsets
    into X, z and the statuses, one fh_collect_columns per batch): iterates, per-column steps, statuses, per-node maxima
    and products equal the reference's for that batch size."""
    kind, m, warm, setting = gc.SWEEPS[case]
    rtol, maxit, restart = setting
    c = gc.sweep_case(kind, m, warm, setting, batch)
    setup_sweep(engine, c, real)
    use_gmres(engine, rtol, 0.0, maxit, restart)
    set_batch(monkeypatch, c, restart, batch)
    out, status, st, counts, node_its = run_sweep(engine, c)
    assert len(c.ref.lock_steps) == -(-len(c.Z) // batch)
    check_sweep("sweep/%s/m=%d/%s/rtol=%g/%s/batch=%d" % (kind, m, "ritz" if warm else "zero", rtol, "real" if real else "complex",
                                                           batch), c, real, out, status, st, counts, node_its)


def test_column_mask_is_ignored(engine):
    """include/feasthip.h: the restarted GMRES path ignores the mask.  The masked call returns the bits of the free one."""
    kind, m, warm, setting = gc.MASK_SWEEP
    rtol, maxit, restart = setting
    c = gc.sweep_case(kind, m, warm, setting)
    setup_sweep(engine, c, True)
    use_gmres(engine, rtol, 0.0, maxit, restart)
    free = run_sweep(engine, c)
    engine.set_column_mask(([1, 0] * m)[:m])
    masked = run_sweep(engine, c)
    check_sweep("mask", c, True, *masked)
    assert np.array_equal(masked[0], free[0]) and np.array_equal(masked[3], free[3])
    assert list(masked[1]) == list(free[1]) and masked[2]["spmm_calls"] == free[2]["spmm_calls"]


@pytest.mark.parametrize("batch", [8, 3])
@pytest.mark.parametrize("case", [0, 2], ids=["converging-and-capped-at-300", "capped-at-12"])
def test_repeated_sweeps_are_bitwise_equal(engine, monkeypatch, case, batch):
    """Three identical sweeps: the same bits, steps, statuses and product counts (fixed-order reductions; the step budget
    and spmm_calls count executed lock-steps, not queued ones)."""
    kind, m, warm, setting = gc.SWEEPS[case]
    rtol, maxit, restart = setting
    c = gc.sweep_case(kind, m, warm, setting, batch)
    setup_sweep(engine, c, True)
    use_gmres(engine, rtol, 0.0, maxit, restart)
    set_batch(monkeypatch, c, restart, batch)
    runs = [run_sweep(engine, c) for _ in range(3)]
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[3], runs[0][3])
        assert list(r[1]) == list(runs[0][1]) and list(r[4]) == list(runs[0][4])
        assert r[2]["spmm_calls"] == runs[0][2]["spmm_calls"] == c.ref.products
