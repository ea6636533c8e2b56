"""Shifted COCG sweep (FEASTHIP_SOLVER_SHIFTED_COCG) on the device: against its step-exact restatement
(shifted_krylov_reference.py; inputs in shifted_cases.py), against the per-node COCG sweep of the same handle, the
fallback paths, bitwise reproducibility and a FEAST solve end to end.

Error model of test_gpu_krylov_steps.py: the device block must lie within kr.tolerance(D) = max(32 D, 64 eps) of the
long-double restatement, D the restatement's own complex128 drift over kr.DRIFT_ORDERS; (node, column) pairs whose stop is
decided by less than 1e-6 are left out.  Converged sweeps (rtol = 1e-10) must agree with solver "cocg" within 32 x the
measured distance between the fused and the five-launch COCG (FH_COCG_FUSED=0, a child process) on the same input.

Measured on an MI355X (119 cases, all pass, none skipped, no pair left out): the device used at most 0.07 of 32 D; shifted
against fused cocg at rtol = 1e-10: 1.7e-10 (zero guess) / 3.6e-9 (warm start), one rank or two, the yardstick fused
against five-launch being 1.2e-10 / 4.6e-9; loops of the FEAST solves, shifted / cocg: 6 / 6 (Laplacian N = 3840), 9 / 9
(N = 50 000), 7 / 7 (tight-binding H).
Discriminating power: what is compared is the SUM over the nodes, and from a zero guess the quadrature-weighted sum is the
contour filter applied to a random vector, which cancels to rounding level.  D is therefore large for the zero-guess cases
of test_sweep_is_the_restatement_step_for_step (2.8 and 5.3 after ONE step with all 16 nodes, 1e-4 .. 1e-3 for
rtol = 3e-2): those pin step counts and statuses.  Their blocks are pinned by test_zero_guess_sweep_under_plain_weights
(every node weighs 1: D of order 1e-11 at most, asserted below 1e-7 / 32), by the single-node families (D <= 9e-15), the warm starts of
the truncated sweeps and the converged comparison with cocg.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import krylov_reference as kr
import shifted_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.environ.get("FH_KRYLOV_STEPS_REPORT")        # measurement runs: the file of test_gpu_krylov_steps.py


@pytest.fixture(autouse=True)
def restore(engine):
    yield
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.set_column_block(0, -1)
    engine.set_column_mask(None)


def setup(engine, c, real, solver="shifted_cocg", rtol=3e-2, maxit=60, **kw):
    engine.set_problem(c.A, None)
    engine.set_contour(c.Zall, c.Wall, c.scale)
    engine.set_node_list(c.nodes)
    engine.set_real_projection(real)
    engine.set_node_solver(None)
    engine.set_solver(solver, rtol=rtol, atol=0.0, maxit=maxit, **kw)


def close_enough(group, dist, D):
    print("shifted-steps %s D=%.3e device=%.3e tol=%.3e" % (group, D, dist, kr.tolerance(D)))
    if REPORT:
        with open(REPORT, "a") as f:
            f.write("shifted/%s %.3e %.3e\n" % (group, D, dist))
    assert dist <= kr.tolerance(D), (group, dist, D)


def test_solver_kind_is_accepted_and_reported(engine):
    """Fails without the feature: feasthip_set_solver(h, 5, ...) is FEASTHIP_ERROR_FPM on the parent."""
    assert engine.lib.feasthip_set_solver(engine.h, 5, 1e-3, 0.0, 50, 30, 64, 1) == 0
    c = sc.sweep_case("lap-N336", "16", 3e-2, 60, 9, True)
    try:
        setup(engine, c, True)
        dP, status, st = engine.contour_apply(engine.upload(c.Q), 9, c.ritz)
        used, seed, seed_its, passes = engine.last_shifted_sweep()
        counts = engine.last_column_iterations(16, 9)
        assert used and seed == c.seed == int(np.argmin(np.abs(c.Zall.imag)))
        assert passes == seed_its == max(c.passes)
        assert counts.max() <= passes <= counts.max() + 1
        assert passes < counts.max(axis=1).sum()                  # not the sum over the nodes
        assert st["spmm_calls"] >= passes
    finally:
        engine.set_node_list(np.arange(16))


def check(group, engine, c, real, out, status):
    assert (~c.decided).sum() <= 0.02 * c.decided.size
    ok = np.flatnonzero(c.col_ok)
    cols = [c.columns[i] for i in ok]
    ref = c.ref.out.real.astype(c.ref.out.dtype) if real else c.ref.out
    close_enough(group, kr.block_dist(out[:, cols], ref[:, ok]), c.drift[real])
    n = len(c.nodes)
    dev = np.asarray(engine.last_column_iterations(n, c.m))[:, c.columns]
    assert np.array_equal(dev[c.decided], c.ref.steps[c.decided]), (group, dev, c.ref.steps)
    if c.decided.all() and len(c.columns) == c.m:
        assert list(status[:n]) == list(c.ref.status), (group, status, c.ref.status)
    used, seed, seed_its, passes = engine.last_shifted_sweep()
    assert used and seed == c.nodes[c.seed]
    if c.decided.all() and len(c.columns) == c.m:
        assert passes == max(c.passes), (group, passes, c.passes)


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("family", list(sc.FAMILIES))
@pytest.mark.parametrize("ld", [16, 32, 64])
@pytest.mark.parametrize("rtol,maxit", [(1e-14, 1), (1e-14, 3), (1e-14, 17), (3e-2, 60), (1e-3, 40)])
def test_sweep_is_the_restatement_step_for_step(engine, rtol, maxit, ld, family, warm):
    """Truncated (maxit = k) and inexact sweeps: Q_proj, per-(node, column) steps and node statuses."""
    m = sc.LD_M[ld]
    c = sc.sweep_case("lap-N1080" if ld == 64 else "lap-N336", family, rtol, maxit, m, warm)
    real = ld != 32
    try:
        setup(engine, c, real, rtol=rtol, maxit=maxit)
        dQ = engine.upload(c.Q)
        dP, status, st = engine.contour_apply(dQ, m, c.ritz)
        tag = "ld=%d/family=%s/rtol=%g/maxit=%d/%s" % (ld, family, rtol, maxit, "ritz" if warm else "zero")
        check(tag, engine, c, real, engine.download(dP, m), status)
        status2, st2 = engine.contour_apply_resident(dQ, m, c.ritz)
        check(tag + "/resident", engine, c, real, engine.download(engine.export_resident(m, which=1), m), status2)
    finally:
        engine.set_node_list(np.arange(16))


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("family", ["3", "16"])
@pytest.mark.parametrize("ld", [32, 64])
@pytest.mark.parametrize("rtol,maxit", sc.INEXACT)
def test_sweep_on_ragged_rows_is_the_restatement(engine, rtol, maxit, ld, family, warm):
    """The inexact sweeps on ragged_pair(331, b_identity=True): rows of 1 to 65 entries and one of N - 10, rows without a
    diagonal, rows without entries (k_spmm at ld 32, k_spmm_row at ld 64, k_shift_vec).  On this matrix the zero-guess sum
    does not cancel (the interval starts inside a cluster of eigenvalues): every case has the discriminating power of
    test_gpu_krylov_steps.py, asserted on the reference here and in test_ragged_cases_host.py."""
    m = sc.LD_M[ld]
    c = sc.sweep_case(sc.RAGGED, family, rtol, maxit, m, warm)
    assert c.decided.all() and c.fp64_steps_agree
    assert 32.0 * max(c.drift.values()) <= sc.POWER, c.drift
    real = ld != 32
    try:
        setup(engine, c, real, rtol=rtol, maxit=maxit)
        dQ = engine.upload(c.Q)
        dP, status, st = engine.contour_apply(dQ, m, c.ritz)
        tag = "ragged/ld=%d/family=%s/rtol=%g/maxit=%d/%s" % (ld, family, rtol, maxit, "ritz" if warm else "zero")
        check(tag, engine, c, real, engine.download(dP, m), status)
        status2, st2 = engine.contour_apply_resident(dQ, m, c.ritz)
        check(tag + "/resident", engine, c, real, engine.download(engine.export_resident(m, which=1), m), status2)
    finally:
        engine.set_node_list(np.arange(16))


@pytest.mark.parametrize("warm", [True, False], ids=["ritz", "zero"])
@pytest.mark.parametrize("ld", [16, 32, 64])
def test_column_mask(engine, ld, warm):
    m = sc.LD_M[ld]
    c = sc.sweep_case("lap-N1080" if ld == 64 else "lap-N336", "16", 3e-2, 60, m, warm, mask=True)
    try:
        setup(engine, c, True)
        engine.set_column_mask(c.mask)
        dP, status, st = engine.contour_apply(engine.upload(c.Q), m, c.ritz)
        counts = engine.last_column_iterations(16, m)
        assert not counts[:, [j for j in range(m) if not c.mask[j]]].any()
        assert counts[:, [j for j in range(m) if c.mask[j]]].any()
        check("mask/ld=%d/%s" % (ld, "ritz" if warm else "zero"), engine, c, True, engine.download(dP, m), status)
    finally:
        engine.set_node_list(np.arange(16))


@pytest.mark.parametrize("family", ["3", "16"])
@pytest.mark.parametrize("ld", [16, 32, 64])
@pytest.mark.parametrize("maxit", [3, 17])
def test_zero_guess_sweep_under_plain_weights(engine, maxit, ld, family):
    """From a zero guess the quadrature-weighted sum is the contour filter of a random vector and cancels to rounding level
    (the module docstring).  With every node weighing 1 the same iterates add up without cancelling: the truncated
    zero-guess sweeps are pinned as blocks here, with the discriminating power test_gpu_krylov_steps.py asks for."""
    m = sc.LD_M[ld]
    c = sc.sweep_case("lap-N1080" if ld == 64 else "lap-N336", family, 1e-14, maxit, m, False, plain_weights=True)
    assert 32.0 * max(c.drift.values()) <= sc.POWER, c.drift
    try:
        setup(engine, c, False, rtol=1e-14, maxit=maxit)
        dP, status, st = engine.contour_apply(engine.upload(c.Q), m, None)
        check("plain-weights/ld=%d/family=%s/maxit=%d" % (ld, family, maxit), engine, c, False, engine.download(dP, m), status)
    finally:
        engine.set_node_list(np.arange(16))


FIVE_LAUNCH_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [{root!r}, os.path.join({root!r}, "oracle"), os.path.join({root!r}, "tests")]
import feastkit_jl_amd as fk
import shifted_cases as sc
eng = fk.HipEngine(0)
res = {{}}
for warm in (0, 1):
    c = sc.Case()
    A, Z, W, _ = sc.problem("lap-N1080")
    Q = fk.seeded_subspace(A.shape[0], 40)
    eng.set_problem(A, None); eng.set_contour(Z, W, 2.0); eng.set_real_projection(True)
    eng.set_solver("cocg", rtol=1e-10, atol=0.0, maxit=1500)
    dP, status, st = eng.contour_apply(eng.upload(Q), 40, sc.ritz_guess("lap-N1080", 40) if warm else None)
    res["out_%d" % warm] = eng.download(dP, 40)
eng.close()
np.savez(sys.argv[1], **res)
print("child ok")
'''


@pytest.fixture(scope="module")
def five_launch(tmp_path_factory):
    """Q_proj of the converged per-node sweeps (zero guess, warm start) through the five-launch COCG, from a child process
    (FH_COCG_FUSED is read once per process)."""
    d = tmp_path_factory.mktemp("five_launch")
    script = d / "five_launch_child.py"
    script.write_text(FIVE_LAUNCH_CHILD.format(root=ROOT))
    out = d / "five.npz"
    p = subprocess.run([sys.executable, str(script), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, FH_COCG_FUSED="0"), timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout.decode(), p.stdout.decode()
    return np.load(out)


def converged_inputs():
    A, Z, W, _ = sc.problem("lap-N1080")
    return A, Z, W, sc.fk.seeded_subspace(A.shape[0], 40)


def fused_cocg_sweep(engine, warm):
    A, Z, W, Q = converged_inputs()
    engine.set_problem(A, None); engine.set_contour(Z, W, 2.0); engine.set_real_projection(True)
    engine.set_node_list(np.arange(16))
    engine.set_node_solver(None)
    engine.set_solver("cocg", rtol=1e-10, atol=0.0, maxit=1500)
    dP, status, _ = engine.contour_apply(engine.upload(Q), 40, sc.ritz_guess("lap-N1080", 40) if warm else None)
    assert not np.any(status)
    return engine.download(dP, 40)


def test_converged_sweep_agrees_with_per_node_cocg(engine, five_launch):
    """rtol = 1e-10: the yardstick is the distance between the two existing COCG forms, fused and five-launch."""
    A, Z, W, Q = converged_inputs()
    for warm in (0, 1):
        fused = fused_cocg_sweep(engine, warm)
        engine.set_solver("shifted_cocg", rtol=1e-10, atol=0.0, maxit=1500)
        dP, status, _ = engine.contour_apply(engine.upload(Q), 40, sc.ritz_guess("lap-N1080", 40) if warm else None)
        shifted = engine.download(dP, 40)
        assert engine.last_shifted_sweep()[0] and not np.any(status)
        yard = kr.block_dist(five_launch["out_%d" % warm], fused)
        dist = kr.block_dist(shifted, fused)
        print("shifted-vs-cocg warm=%d: fused vs five-launch %.3e, shifted vs fused %.3e" % (warm, yard, dist))
        assert dist <= 32.0 * yard, (warm, dist, yard)


TWO_RANK_WORKER = r'''
import os, sys
sys.path[:0] = [r"{root}", r"{root}/oracle", r"{root}/tests"]
import numpy as np, torch, torch.distributed as dist
import feastkit_jl_amd as fk
import shifted_cases as sc
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=rank, world_size=2)
A, Z, W, _ = sc.problem("lap-N1080")
Q = fk.seeded_subspace(A.shape[0], 40)
eng = fk.HipEngine(0)
eng.comm_init_from_group(None)
res = {{}}
for warm in (0, 1):
    eng.set_problem(A, None); eng.set_contour(Z, W, 2.0); eng.set_real_projection(True)
    eng.set_node_range(8 * rank, 8)                      # node groups: rank 0 sweeps nodes 0 .. 7, rank 1 nodes 8 .. 15
    eng.set_solver("shifted_cocg", rtol=1e-10, atol=0.0, maxit=1500)
    dP, status, st = eng.contour_apply(eng.upload(Q), 40, sc.ritz_guess("lap-N1080", 40) if warm else None)
    res["out_%d" % warm] = eng.download(dP, 40)          # summed over the ranks inside the call
    res["status_%d" % warm] = np.asarray(status)
    res["shifted_%d" % warm] = np.array(eng.last_shifted_sweep(), dtype=np.int64)
eng.close()
# the driver: stats["shifted"] of every loop names this rank's own seed
eng = fk.HipEngine(0)
Al, lam = fk.workloads.laplacian_3d_standard(16, 12, 10)
fpm = fk.feastinit(); fpm[2] = 16; fpm[4] = 40
r = fk.feast_hip_hermitian(eng, Al, None, 0.0, 0.42, 32, fpm, solver="shifted_cocg", warm_start=True, inner_rtol=3e-2,
                           solver_maxiter=100, node_assignment="block", real_projection=True)
res["feast"] = np.array([r.info, r.M, r.epsout, r.loop] + list(np.sort(r.lambda_)), dtype=float)
res["feast_local_nodes"] = np.array(r.stats["local_nodes"])
res["feast_seeds"] = np.array([[int(e["used"]), e["seed_node"]] for e in r.stats["shifted"]])
eng.close()
np.savez(r"{out}/rank%d.npz" % rank, **res)
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_on_one_card(engine, five_launch, tmp_path):
    """Node groups over the shared-device transport: the sum of the two ranks' shifted sweeps (each rank its own family and
    seed) equals the one-rank cocg sweep within the converged-sweep bound, and stats["shifted"] names each rank's seed."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "two_rank_worker.py"
    script.write_text(TWO_RANK_WORKER.format(root=ROOT, port=port, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    got = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    A, Z, W, Q = converged_inputs()
    for warm in (0, 1):
        fused = fused_cocg_sweep(engine, warm)
        yard = kr.block_dist(five_launch["out_%d" % warm], fused)
        assert got[0]["out_%d" % warm].tobytes() == got[1]["out_%d" % warm].tobytes()      # one all-reduce: the same sum on both
        dist = kr.block_dist(got[0]["out_%d" % warm], fused)
        print("shifted-two-ranks warm=%d: fused vs five-launch %.3e, two-rank shifted vs one-rank cocg %.3e" % (warm, yard, dist))
        assert dist <= 32.0 * yard, (warm, dist, yard)
        for r in range(2):
            nodes = np.arange(8 * r, 8 * r + 8)
            used, seed, seed_its, passes = got[r]["shifted_%d" % warm]
            assert used == 1 and seed == nodes[int(np.argmin(np.abs(Z[nodes].imag)))] and passes == seed_its > 0
            assert not got[r]["status_%d" % warm].any()
    Al, lam = sc.fk.workloads.laplacian_3d_standard(16, 12, 10)
    inside = lam[(lam >= 0) & (lam <= 0.42)]
    assert np.array_equal(got[0]["feast"], got[1]["feast"])
    f = got[0]["feast"]
    assert (int(f[0]), int(f[1])) == (0, len(inside)) and f[2] <= 1e-12
    assert np.abs(f[4:4 + len(inside)] - inside).max() <= 1e-10
    Zf, _ = sc.contour16(0.0, 0.42)
    Zf = np.asarray(Zf)
    for r in range(2):
        nodes = got[r]["feast_local_nodes"]
        assert len(nodes) == 8 and not set(nodes) & set(got[1 - r]["feast_local_nodes"])
        want = nodes[int(np.argmin(np.abs(Zf[nodes].imag)))]
        assert len(got[r]["feast_seeds"]) >= int(f[3]) and all(u == 1 and sd == want for u, sd in got[r]["feast_seeds"])


@pytest.mark.parametrize("path", ["B-given", "complex-A", "factor-precision-32", "moments"])
def test_fallback_is_the_cocg_sweep_bit_for_bit(engine, path):
    """used = 0 and the output, statuses and step counts of solver "cocg", bit for bit.  complex-A: cocg refuses complex
    input (it needs a complex-symmetric shifted matrix), so what is compared there is the refusal, the same message."""
    A, Z, W, _ = sc.problem("lap-N336")
    N = A.shape[0]
    B = None
    if path == "B-given":
        B = sp.identity(N, format="csr") + 0.1 * A
    if path == "complex-A":
        A = sp.csr_matrix(A.astype(np.complex128))
    Q = sc.fk.seeded_subspace(N, 9)
    ritz = sc.ritz_guess("lap-N336", 9)
    got = {}
    for solver in ("cocg", "shifted_cocg"):
        engine.set_problem(A, B); engine.set_contour(Z, W, 2.0); engine.set_real_projection(True)
        engine.set_node_solver(None)
        engine.set_solver(solver, rtol=3e-2, atol=0.0, maxit=60, factor_precision=32 if path == "factor-precision-32" else 64)
        try:
            r = engine.contour_apply(engine.upload(Q), 9, ritz, want_moments=(path == "moments"))
            got[solver] = ("ok", engine.download(r[0], 9), list(r[1]), engine.last_column_iterations(16, 9).copy())
        except sc.fk.FeastHipError as e:
            got[solver] = ("error", str(e))
        assert engine.last_shifted_sweep()[0] is False
    a, b = got["cocg"], got["shifted_cocg"]
    assert a[0] == b[0], (a[0], b[0])
    if a[0] == "ok":
        assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and np.array_equal(a[3], b[3])
    else:
        assert a[1] == b[1]


def test_two_sweeps_are_bitwise_identical(engine):
    c = sc.sweep_case("lap-N1080", "16", 3e-2, 60, 40, True)
    try:
        setup(engine, c, True)
        dQ = engine.upload(c.Q)
        a = engine.download(engine.contour_apply(dQ, 40, c.ritz)[0], 40)
        ia = engine.last_column_iterations(16, 40).copy()
        b = engine.download(engine.contour_apply(dQ, 40, c.ritz)[0], 40)
        assert a.tobytes() == b.tobytes()
        assert np.array_equal(ia, engine.last_column_iterations(16, 40))
    finally:
        engine.set_node_list(np.arange(16))


def _host_residual(A, lam, X):
    R = A @ X - X * lam[None, :]
    return float((np.linalg.norm(R, axis=0) / np.maximum(np.linalg.norm(X, axis=0) * max(abs(lam).max(), 1.0), 1e-300)).max())


def _laplacian(dims, interval):
    A, lam = sc.fk.workloads.laplacian_3d_standard(*dims)
    return A, lam[(lam >= interval[0]) & (lam <= interval[1])], interval


def _tight_binding_top():
    """The tight-binding H of test_gpu_direct_pivoting.py (N = 3840, zero diagonal, spectrum symmetric about E = 0) with
    the interval that holds its six largest eigenvalues: off E = 0, at the upper end of the spectrum."""
    from test_gpu_direct_pivoting import bipartite_hamiltonian
    H = bipartite_hamiltonian((16, 16, 15), 51)
    lam = np.linalg.eigvalsh(H.toarray())
    return H, lam[-6:], (0.5 * (lam[-7] + lam[-6]), lam[-1] + 0.5 * (lam[-1] - lam[-6]))


E2E = {
    # name -> (builder of (A, eigenvalues inside, interval), M0, fpm[18] or None, iteration cap)
    "laplacian-N3840": (lambda: _laplacian((20, 16, 12), (0.1, 0.32)), None, None, 100),
    "laplacian-N50000": (lambda: _laplacian((50, 40, 25), (0.0, 0.1775 / (1.0 - 0.1 * 0.1775))), 64, 4000, 50),   # the bench's window, contour and cap
    "tight-binding-N3840": (_tight_binding_top, 16, None, 100),
}


@pytest.mark.parametrize("name", list(E2E))
def test_feast_end_to_end(name):
    """fk.feast(A, interval, solver="shifted_cocg") in the inexact mode: M and eigenvalues of the closed form (the dense
    spectrum for the tight-binding H), the parity bars of the residuals, and the loop count of solver="cocg" +- 1.
    Measured on an MI355X, loops shifted / cocg: see the print."""
    fk = sc.fk
    build, M0, aspect, cap = E2E[name]
    A, inside, interval = build()
    assert 4 <= len(inside) <= 48
    res = {}
    for solver in ("cocg", "shifted_cocg"):
        fpm = fk.feastinit()
        fpm[2] = 16
        if aspect is not None:
            fpm[16], fpm[18] = 0, aspect
        res[solver] = fk.feast(A, None, interval, M0=M0 or int(1.5 * len(inside)) + 8, fpm=fpm, solver=solver, warm_start=True,
                               inner_rtol=3e-2, solver_maxiter=cap)
    r, r0 = res["shifted_cocg"], res["cocg"]
    print("shifted-feast %s loops: shifted %d, cocg %d; epsout %.2e / %.2e" % (name, r.loop, r0.loop, r.epsout, r0.epsout))
    assert r.info == 0 and r.M == len(inside)
    assert np.abs(np.sort(r.lambda_) - inside).max() <= 1e-10
    assert r.epsout <= 1e-12
    order = np.argsort(r.lambda_)
    assert _host_residual(A, np.asarray(r.lambda_)[order], np.asarray(r.q)[:, order]) <= 1e-10
    assert abs(r.loop - r0.loop) <= 1
    assert all(s["used"] for s in r.stats["shifted"]) and len(r.stats["shifted"]) >= r.loop
    assert "shifted" not in r0.stats
