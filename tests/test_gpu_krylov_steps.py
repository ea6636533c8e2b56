"""Truncated and inexact Krylov solves of the device against the step-exact per-column restatement
(krylov_reference.py; inputs and reference results in krylov_cases.py).

Every case compares the returned block with the long-double reference iterate / sweep, the step counts and the status
codes.  The tolerance is measured at test time: D = the drift of the restatement itself in complex128 over four summation
orders against long double, and the device must lie within max(32 D, 64 eps) (krylov_reference.tolerance).  (node, column)
pairs whose stop is decided by less than 1e-6 are left out, at most 2 % of a case.

Measured on an MI355X (105 cases, all pass, none skipped, no pair left out); per group the largest D, the largest distance
of the device from the long-double reference, and the largest share of its tolerance the device used:

    truncated cocg, far shift          D <= 5.0e-13   device <= 5.9e-14   0.07
    truncated cocg, node next to Emax  D <= 5.6e-10   device <= 6.1e-10   0.05
    truncated bicgstab, far shift      D <= 7.5e-11   device <= 2.0e-11   0.04
    truncated bicgstab, near (k <= 3)  D <= 2.3e-09   device <= 3.6e-10   0.03
    own stop step, fused cocg          D <= 9.5e-16   device <= 1.4e-15   0.09
    own stop step, five-launch cocg    D <= 7.5e-16   device <= 5.0e-16   0.03
    own stop step, bicgstab            D <= 3.7e-11   device <= 2.9e-11   0.04
    inexact cocg sweeps (96)           D <= 1.7e-09   device <= 7.5e-10   0.06
    start paths (20)                   D <= 1.7e-09   device <= 7.5e-10   0.05
    five-launch sweeps (child)         D <= 9.3e-11   device <= 6.7e-11   0.07
    bicgstab sweeps                    D <= 2.0e-11   device <= 2.0e-12   0.03
    mask / node list / column block    D <= 5.4e-15   device <= 7.2e-15   0.05

On the ragged pencils of ragged_cases.py (70 more cases: rows of 0 to 65 entries and one of N - 1, missing diagonals,
N = 47 / 323 / 331; the whole report is profiles/ragged_krylov_steps.txt):

    truncated cocg, far shift          D <= 3.9e-12   device <= 1.8e-12   0.04
    truncated cocg, node next to Emax  D <= 7.0e-10   device <= 7.7e-10   0.07
    truncated bicgstab, far / near     D <= 1.1e-12   device <= 1.0e-12   0.03
    inexact cocg sweeps (96)           D <= 3.3e-10   device <= 5.0e-11   0.03
    start paths (12)                   D <= 3.3e-10   device <= 9.2e-11   0.03

The device never needed more than a tenth of 32 D.  BiCGStab's own drift limits how far its cases can be cut (see
krylov_cases.py: k <= 17 far from the spectrum for the two larger pencils, k <= 3 next to it, 5 steps for the Hermitian
sweep): beyond that 32 D passes 1e-7 and the comparison would no longer tell a defect from rounding.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.environ.get("FH_KRYLOV_STEPS_REPORT")        # measurement runs: a file to append "group D distance" lines to


def close_enough(group, dist, D):
    print("krylov-steps %s D=%.3e device=%.3e tol=%.3e" % (group, D, dist, kr.tolerance(D)))
    if REPORT:
        with open(REPORT, "a") as f:
            f.write("%s %.3e %.3e\n" % (group, D, dist))
    assert 32.0 * D <= kc.POWER, (group, D)              # a condition on the reference alone
    assert dist <= kr.tolerance(D), (group, dist, D)


def use_solver(engine, solver, rtol, atol, maxit, **kw):
    engine.set_node_solver(None)
    engine.set_column_mask(None)
    engine.set_solver(solver, rtol=rtol, atol=atol, maxit=maxit, **kw)


@pytest.fixture(autouse=True)
def restore(engine):
    yield
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.set_column_block(0, -1)


# ---- truncated single-shift solves -----------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("name", list(kc.TRUNC))
def test_truncated_solve_is_the_kth_iterate(engine, name, near):
    """maxit = k, rtol = 1e-14: rc 5 and Y is the reference's k-th iterate, krylov_iterations = k per 64-column panel;
    where the reference reaches the target before step k: rc 0, its stop step and its iterate at that step."""
    import torch
    c = kc.trunc_case(name, near)
    try:
        engine.set_problem(c.A, c.B)
        dX = engine.upload(c.X)
        use_solver(engine, c.solver, 1e-14, 0.0, 1)
        engine.shifted_solve(c.z, dX, c.m)
    except (torch.cuda.OutOfMemoryError, kc.fk.FeastHipError) as e:
        if c.N > 50000 and "memory" in str(e).lower():
            pytest.skip("not enough device memory for %s: %s" % (name, e))
        raise
    npanels = (c.m + 63) // 64
    for k in c.ks:
        use_solver(engine, c.solver, 1e-14, 0.0, k)
        dY, rc = engine.shifted_solve(c.z, dX, c.m)
        Y = engine.download(dY)
        its = engine.last_stats["krylov_iterations"]
        want = [kr.truncated(r, k) for r in c.ref]       # (x, steps, status, active, margin)
        decided = [w[4] >= kc.MARGIN_MIN for w in want]
        assert sum(not d for d in decided) <= kc.LEFT_OUT_MAX * len(want)
        if all(decided):
            by_panel = [[w for j, w in zip(c.columns, want) if j // 64 == p] for p in range(npanels)]
            if all(any(w[3] for w in p) for p in by_panel):
                # a column of every panel is still active: rc 5, and the panel's count is k whatever the others did
                assert rc == kr.NO_CONVERGENCE and its == k * npanels, (name, k, rc, its)
            elif len(c.columns) == c.m:
                assert rc == (kr.NO_CONVERGENCE if any(w[3] for w in want) else 0), (name, k, rc)
                assert its == sum(max(w[1] for w in p) for p in by_panel), (name, k, its)
        dist = max(kr.rel_dist(Y[:, j], w[0]) for j, w, ok in zip(c.columns, want, decided) if ok)
        close_enough("truncated/%s/%s/k=%d" % (name, "near" if near else "far", k), dist, c.drift[k])


# ---- columns that stop at different steps ----------------------------------------------------------------------------
@pytest.mark.parametrize("rtol,atol", kc.STOP_SETTINGS)
@pytest.mark.parametrize("solver,method,dense", kc.STOP_SOLVERS, ids=[s[1] for s in kc.STOP_SOLVERS])
def test_every_column_stops_at_its_own_step(engine, solver, method, dense, rtol, atol):
    """Each column of Y is the reference iterate at that column's own stop step (the last-step rule); the zero column and
    the column below atol come back as zeros."""
    c = kc.stop_case(method, rtol, atol)
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= kc.LEFT_OUT_MAX * c.m
    engine.set_problem(c.A, c.B)
    use_solver(engine, solver, rtol, atol, 400)
    dY, rc = engine.shifted_solve(c.z, engine.upload(c.X), c.m)
    Y = engine.download(dY)
    assert rc == 0
    assert not Y[:, 5].any()
    if atol > 0:
        assert not Y[:, 11].any()
    if c.decided.all():
        assert engine.last_stats["krylov_iterations"] == max(r.steps for r in c.ref)
    for j in np.flatnonzero(c.decided):
        if c.ref[j].steps:
            close_enough("stops/%s/rtol=%g/atol=%g/col=%d/step=%d" % (method, rtol, atol, j, c.ref[j].steps),
                         kr.rel_dist(Y[:, j], c.ref[j].x), c.drift[j])


# ---- inexact contour sweeps ------------------------------------------------------------------------------------------
def setup_sweep(engine, c, real):
    engine.set_problem(c.A, c.B)
    engine.set_contour(c.Z, c.W, c.scale)
    engine.set_real_projection(real)
    engine.set_column_block(0, -1)


def check_sweep(group, c, out, status, real, counts=None, node_its=None, stats=None):
    """``out``: the device's N x m block.  Columns with an undecidable pair are left out (at most 2 % of the pairs)."""
    assert c.fp64_steps_agree
    assert (~c.decided).sum() <= kc.LEFT_OUT_MAX * c.decided.size
    ok = np.flatnonzero(c.col_ok)
    cols = [c.columns[i] for i in ok]
    ref = kc.project(c.ref.out, real)[:, ok]
    close_enough(group, kr.block_dist(out[:, cols], ref), c.drift[real])
    whole = c.decided.all() and len(c.columns) == c.m
    if whole:
        assert list(status[:len(c.Z)]) == list(c.ref.status), (group, status, c.ref.status)
    if counts is not None:
        dev = np.asarray(counts)[:, c.columns]
        assert np.array_equal(dev[c.decided], c.ref.steps[c.decided]), (group, dev, c.ref.steps)
    if whole:
        rowmax = c.ref.steps.max(axis=1)
        if node_its is not None:
            assert list(node_its) == list(rowmax), (group, node_its, rowmax)
        if stats is not None:
            assert stats["krylov_iterations"] == rowmax.sum(), (group, stats, rowmax)


# the full grid of widths on cfg 3; the ragged pencils (krylov_cases.sweep_problem) at one k_spmm width and the full one
SWEEP_GRID = [("cfg3", m) for m in kc.SWEEP_M] + [(kind, m) for kind in kc.SWEEP_KINDS[1:] for m in kc.RAGGED_SWEEP_M]


@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("kind,m", SWEEP_GRID, ids=[str(m) if kind == "cfg3" else "%s-%d" % (kind, m) for kind, m in SWEEP_GRID])
@pytest.mark.parametrize("rtol,maxit", kc.SWEEP_SETTINGS)
def test_inexact_cocg_sweep(engine, rtol, maxit, kind, m, warm, real):
    c = kc.sweep_case("cocg_fused", rtol, maxit, m, warm, kind=kind)
    setup_sweep(engine, c, real)
    use_solver(engine, "cocg", rtol, 0.0, maxit)
    dQ = engine.upload(c.Q)
    tag = "sweep/cocg/%srtol=%g/maxit=%d/m=%d/%s/%s" % ("" if kind == "cfg3" else kind + "/", rtol, maxit, m, "ritz" if warm else "zero",
                                                        "real" if real else "complex")
    n = len(c.Z)
    dP, status, st = engine.contour_apply(dQ, m, c.ritz)
    check_sweep(tag, c, engine.download(dP, m), status, real, engine.last_column_iterations(n, m),
                engine.last_node_iterations(n), st)
    if c.decided.all() and len(c.columns) == m:
        # fh_krylov: one product per queued iteration of the fused form and none for the start residual of a shared start;
        # the host queues chunks of 16 until it has seen every column stop: no fewer than the longest column's steps (plus
        # the product in which that column's true norm is seen, unless it stopped on the estimate or at the cap)
        assert c.ref.steps.max() <= st["spmm_calls"] <= maxit, (tag, st)
    status2, st2 = engine.contour_apply_resident(dQ, m, c.ritz)
    out2 = engine.download(engine.export_resident(m, which=1), m)
    check_sweep(tag + "/resident", c, out2, status2, real, engine.last_column_iterations(n, m), engine.last_node_iterations(n), st2)


PATHS = {"lazy": {}, "no-lazy": {"FH_NO_LAZY_START": "1"}, "no-shared": {"FH_NO_SHARED_START": "1"}}
PATH_GRID = [(p, "cfg3") for p in list(PATHS) + ["moments", "no-sum-mode"]] + [(p, "ragged") for p in PATHS]


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("path,kind", PATH_GRID, ids=[p if kind == "cfg3" else "%s-%s" % (kind, p) for p, kind in PATH_GRID])
@pytest.mark.parametrize("rtol,maxit", kc.SWEEP_SETTINGS[:2])
def test_start_paths_meet_the_same_reference(engine, monkeypatch, rtol, maxit, path, kind, warm):
    """Lazy start (default), materialised shared start, per-node start residuals, and the two forms without the shared
    accumulator (moments requested; FH_NO_SUM_MODE=1, read when a handle is created).  The first three also on the ragged
    pencil with B: the column-scaled first product (colscale) over rows of every length."""
    import feastkit_jl_amd as fk
    c = kc.sweep_case("cocg_fused", rtol, maxit, 24, warm, kind=kind)
    for k, v in PATHS.get(path, {}).items():
        monkeypatch.setenv(k, v)
    eng = engine
    if path == "no-sum-mode":
        monkeypatch.setenv("FH_NO_SUM_MODE", "1")
        eng = fk.HipEngine(0)
    try:
        setup_sweep(eng, c, True)
        use_solver(eng, "cocg", rtol, 0.0, maxit)
        r = eng.contour_apply(eng.upload(c.Q), 24, c.ritz, want_moments=(path == "moments"))
        n = len(c.Z)
        check_sweep("paths/%s%s/rtol=%g/%s" % ("" if kind == "cfg3" else kind + "/", path, rtol, "ritz" if warm else "zero"), c, eng.download(r[0], 24), r[1], True,
                    eng.last_column_iterations(n, 24), eng.last_node_iterations(n), r[2])
        if c.decided.all():
            first = 0 if path in ("lazy", "no-lazy") else 1        # the start residual is a product of its own
            assert c.ref.steps.max() + first <= r[2]["spmm_calls"] <= maxit + first, (path, r[2])
    finally:
        if eng is not engine:
            eng.set_solver("direct")
            eng.close()


CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [{root!r}, os.path.join({root!r}, "oracle"), os.path.join({root!r}, "tests")]
import feastkit_jl_amd as fk
import krylov_cases as kc
eng = fk.HipEngine(0)
res = {{}}
A, B, Z, W, scale = kc.sweep_problem()
Q = fk.seeded_subspace(A.shape[0], 24)
for i, (rtol, maxit) in enumerate(kc.SWEEP_SETTINGS[:2]):
    for warm in (True, False):
        eng.set_problem(A, B); eng.set_contour(Z, W, scale); eng.set_real_projection(True)
        eng.set_solver("cocg", rtol=rtol, atol=0.0, maxit=maxit)
        dP, status, st = eng.contour_apply(eng.upload(Q), 24, kc.sweep_ritz(24) if warm else None)
        key = "%d_%d" % (i, int(warm))
        res["out_" + key] = eng.download(dP, 24)
        res["status_" + key] = status
        res["cols_" + key] = eng.last_column_iterations(len(Z), 24)
        res["its_" + key] = np.array([st["krylov_iterations"], st["spmm_calls"]])
eng.close()
np.savez(sys.argv[1], **res)
print("child ok")
'''


def test_five_launch_cocg_sweep_in_a_child_process(tmp_path):
    """FH_COCG_FUSED=0 is read once per process: a fresh child runs the sweeps through the five-launch form (sum mode of
    k_cocg_p_sum, the `accum` flag of k_fin_alpha), the parent compares them with the five-launch restatement."""
    script = tmp_path / "five_launch_child.py"
    script.write_text(CHILD.format(root=ROOT))
    out = tmp_path / "five_launch.npz"
    p = subprocess.run([sys.executable, str(script), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, FH_COCG_FUSED="0"), timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout.decode(), p.stdout.decode()
    got = np.load(out)
    for i, (rtol, maxit) in enumerate(kc.SWEEP_SETTINGS[:2]):
        for warm in (True, False):
            c = kc.sweep_case("cocg5", rtol, maxit, 24, warm)
            key = "%d_%d" % (i, int(warm))
            check_sweep("five-launch/rtol=%g/%s" % (rtol, "ritz" if warm else "zero"), c, got["out_" + key], got["status_" + key],
                        True, got["cols_" + key], None, {"krylov_iterations": int(got["its_" + key][0])})


@pytest.mark.parametrize("kind,real,maxit", kc.BICGSTAB_SWEEPS)
def test_inexact_bicgstab_sweep(engine, kind, real, maxit):
    c = kc.sweep_case("bicgstab", 3e-2, maxit, 24, True, kind=kind)
    setup_sweep(engine, c, real)
    use_solver(engine, "bicgstab", 3e-2, 0.0, maxit)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), 24, c.ritz)
    n = len(c.Z)
    check_sweep("sweep/bicgstab/%s/%s" % (kind, "real" if real else "complex"), c, engine.download(dP, 24), status, real,
                engine.last_column_iterations(n, 24), engine.last_node_iterations(n), st)
    if c.decided.all():
        # the start residual, then two products per queued iteration
        assert 1 + 2 * c.ref.steps.max() <= st["spmm_calls"] <= 1 + 2 * maxit
        assert st["spmm_calls"] % 2 == 1


def test_column_mask_under_the_inexact_sweep(engine):
    """Masked columns keep the closed-form warm start sum_e w_e q_c / (z_e - lambda_c), the others are the reference
    iterates; the mask holds for one call."""
    c = kc.sweep_case("cocg_fused", 3e-2, 50, 24, True, mask=True)
    free = kc.sweep_case("cocg_fused", 3e-2, 50, 24, True)
    n = len(c.Z)
    setup_sweep(engine, c, True)
    use_solver(engine, "cocg", 3e-2, 0.0, 50)
    dQ = engine.upload(c.Q)
    engine.set_column_mask(c.mask)
    dP, status, st = engine.contour_apply(dQ, 24, c.ritz)
    counts = engine.last_column_iterations(n, 24)
    out = engine.download(dP, 24)
    assert not counts[:, 1::2].any()
    check_sweep("mask", c, out, status, True, counts, engine.last_node_iterations(n), st)
    closed = sum(c.scale * w / (z - c.ritz[None, 1::2]) for z, w in zip(c.Z, c.W)).real * c.Q[:, 1::2]
    close_enough("mask/closed-form", kr.block_dist(out[:, 1::2], closed), c.drift[True])
    dP, status, st = engine.contour_apply(dQ, 24, c.ritz)          # the mask is gone
    check_sweep("mask/next-call", free, engine.download(dP, 24), status, True, engine.last_column_iterations(n, 24))


def test_node_list_and_column_block_add_up(engine):
    c = kc.sweep_case("cocg_fused", 3e-2, 50, 40, True, all_columns=True)
    setup_sweep(engine, c, False)
    use_solver(engine, "cocg", 3e-2, 0.0, 50)
    dQ = engine.upload(c.Q)
    groups = ([6, 1, 4], [7, 0], [3, 5, 2])                # a permuted split of the 8 nodes
    total = np.zeros((c.A.shape[0], 40), dtype=np.complex128)
    try:
        for g in groups:
            engine.set_node_list(g)
            dP, status, st = engine.contour_apply(dQ, 40, c.ritz)
            total += engine.download(dP, 40)
            counts = engine.last_column_iterations(len(g), 40)
            want, dec = c.ref.steps[g], c.decided[g]
            assert np.array_equal(counts[dec], want[dec]), (g, counts, want)
            if c.decided.all():
                assert list(status[:len(g)]) == list(c.ref.status[g])
                assert st["krylov_iterations"] == want.max(axis=1).sum()
    finally:
        engine.set_node_list(np.arange(8))
    check_sweep("node-list/sum", c, total, c.ref.status, False)
    engine.set_column_block(16, 16)                        # columns 16 .. 31 only: zero elsewhere
    dP, status, st = engine.contour_apply(dQ, 40, c.ritz)
    engine.set_column_block(0, -1)
    part = engine.download(dP, 40)
    assert not part[:, :16].any() and not part[:, 32:].any()
    ok = [j for j in range(16, 32) if c.col_ok[j]]
    close_enough("column-block", kr.block_dist(part[:, ok], c.ref.out[:, ok]), c.drift[False])
    counts = engine.last_column_iterations(8, 16)
    assert np.array_equal(counts[c.decided[:, 16:32]], c.ref.steps[:, 16:32][c.decided[:, 16:32]])


def test_complex64_correction_sweep_takes_the_reference_steps(engine):
    """factor_precision = 32: step counts and statuses of the inexact COCG sweep equal the fp64 reference's on the columns
    whose decision margin is above 1e-3 (the iterates are out of scope: complex64 needs an error model of its own)."""
    c = kc.sweep_case("cocg_fused", 3e-2, 50, 24, True)
    setup_sweep(engine, c, True)
    use_solver(engine, "cocg", 3e-2, 0.0, 50, factor_precision=32)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), 24, c.ritz)
    counts = engine.last_column_iterations(len(c.Z), 24)
    sure = c.ref.margin > 1e-3
    assert sure.mean() > 0.5
    assert np.array_equal(counts[sure], c.ref.steps[sure]), (counts, c.ref.steps)
    if sure.all():
        assert list(status[:len(c.Z)]) == list(c.ref.status)
