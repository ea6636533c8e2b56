"""Shift-preconditioned GMRES (feasthip_set_preconditioner; fh_gmres with a preconditioner in csrc/fh_api.hip, k_precond_op in
csrc/fh_sparse.hip) against its step-exact restatement (precond_reference.py; cases in precond_cases.py), the factor
accounting, the drivers end to end, the untouched plain path, and every refusal.

The comparison is that of test_gpu_gmres_steps.py: the summed block within max(32 D, 64 eps) of the long-double reference
(D: the restatement's own complex128 drift, the factors' rounding included), per-(node, column) step counts, statuses,
lock-steps, operator products and substitution sweeps equal; pairs whose stop is decided by less than MARGIN_MIN are left
out (none is, in these cases)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import feast_oracle as fo
import feastkit_jl_amd as fk
import gmres_cases as gc
import krylov_reference as kr
import precond_cases as pc
from feastkit_jl_amd.ingest import polynomial_union_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("FH_MF", "FH_MF_MAX_MULTIPLIER", "FH_WBAND", "FH_GMRES_BUDGET_MB")


@pytest.fixture(autouse=True)
def restore(engine, monkeypatch):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    engine._problem_fp = None                # every test plans for itself, whatever plan a knob left on the engine
    yield
    engine.set_preconditioner(None)
    engine.set_node_solver(None)
    engine.set_adjoint(False)
    engine.set_solver("direct")
    engine.set_real_projection(False)
    engine.free_factors()
    engine._problem_fp = None


def close_enough(group, dist, D):
    print("precond %s D=%.3e device=%.3e tol=%.3e" % (group, D, dist, kr.tolerance(D)))
    assert 32.0 * D <= pc.POWER, (group, D)              # a condition on the reference alone
    assert dist <= kr.tolerance(D), (group, dist, D)


def setup(engine, c, real=False, maxit=pc.MAXIT, precond=True):
    engine.set_problem(c.A, c.B)
    engine.set_contour(c.Z, c.W, c.scale)
    engine.set_real_projection(real)
    engine.set_node_solver(None)
    engine.set_solver("gmres", rtol=pc.RTOL, atol=0.0, maxit=maxit, restart=c.restart)
    if precond:
        engine.set_preconditioner(c.pivots, c.node_pivot)


def run(engine, c):
    n = len(c.Z)
    dP, status, st = engine.contour_apply(engine.upload(c.Q), c.m, c.ritz)
    return (engine.download(dP, c.m), list(status[:n]), st, engine.last_column_iterations(n, c.m), list(engine.last_node_iterations(n)),
            engine.last_precond_sweep())


def check(group, c, real, got, want_out, want_steps, want_status, want_margin, want_products, want_sweeps, D):
    out, status, st, counts, node_its, last = got
    decided = want_margin >= pc.MARGIN_MIN
    assert (~decided).sum() <= pc.LEFT_OUT_MAX * decided.size
    ok = np.flatnonzero(decided.all(axis=0))
    cols = [c.columns[i] for i in ok]
    close_enough(group, kr.block_dist(out[:, cols], pc.project(want_out, real)[:, ok]), D)
    dev = np.asarray(counts)[:, c.columns]
    assert np.array_equal(dev[decided], want_steps[decided]), (group, dev, want_steps)
    assert last["used"] and last["pivots"] == len(c.pivots) and not last["fell_back"]
    if decided.all() and len(c.columns) == c.m:
        rowmax = want_steps.max(axis=1)
        assert status == list(want_status), (group, status, want_status)
        assert node_its == list(rowmax), (group, node_its, rowmax)
        assert st["krylov_iterations"] == rowmax.sum()
        assert st["spmm_calls"] == want_products, (group, st, want_products)
        assert last["substitution_sweeps"] == want_sweeps, (group, last, want_sweeps)


# ---- 1. step parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_preconditioned_sweep_follows_the_reference(engine, name, real):
    c = pc.case(name)
    assert c.fp64_steps_agree
    setup(engine, c, real)
    r = c.ref
    check("sweep/%s/%s" % (name, "real" if real else "complex"), c, real, run(engine, c), r.out, r.steps, r.status, r.margin,
          r.products, r.sweeps, c.drift[real])


@pytest.mark.parametrize("name", [n for n in pc.CASES if pc.CASES[n][6]])
def test_truncated_sweep_is_the_kth_iterate(engine, name):
    """maxit = k in {1, mr, mr + 1}: inside the first cycle, exactly at its end, one step into the second."""
    c = pc.case(name)
    for k in c.ks:
        setup(engine, c, False, maxit=k)
        out, steps, status, margin, products, sweeps = c.trunc[k]
        assert status.any()                                   # the cap cuts the sweep short
        check("truncated/%s/k=%d" % (name, k), c, False, run(engine, c), out, steps, status, margin, products, sweeps, c.trunc_drift[k])


@pytest.mark.parametrize("plan", ["multifrontal", "band", "fallback"])
def test_every_direct_plan_serves_the_pivots(engine, monkeypatch, plan):
    """The pivot factors under the multifrontal plan, the blocked band plan, and the band plan the multifrontal LU falls back
    to when it rejects a pivot (a normal outcome, flagged): the same reference.  (The narrow band plan: the tridiagonal case.)"""
    c = pc.case("cfg3-N336-m16-r10")
    monkeypatch.setenv("FH_MF", "0" if plan == "band" else "1")
    if plan == "fallback":
        monkeypatch.setenv("FH_MF_MAX_MULTIPLIER", "0")
    setup(engine, c)
    assert engine.band_plan()[3] == (1 if plan == "band" else 2)
    got = run(engine, c)
    assert got[5]["fell_back"] == (plan == "fallback")
    assert engine.band_plan()[3] == (2 if plan == "multifrontal" else 1)
    got[5]["fell_back"] = False
    r = c.ref
    check("plan/" + plan, c, False, got, r.out, r.steps, r.status, r.margin, r.products, r.sweeps, c.drift[False])


def test_tridiagonal_case_takes_the_narrow_band_plan(engine):
    setup(engine, pc.case("tridiag-I-N150-m3-r30"))
    assert engine.band_plan()[3] == 0 and engine.band_plan()[:2] == (1, 1)


def test_shifted_solve_takes_the_nearest_pivot(engine):
    """feasthip_shifted_solve under the setting: one node, the nearest pivot, the reference's column of that node."""
    c = pc.case("csr-B-N333-m5-r30")
    setup(engine, c)
    e = 3
    X = np.stack([np.asarray(col.b, dtype=np.complex128) for col in c.ref.cols[e]], axis=1)
    dY, rc = engine.shifted_solve(c.Z[e], engine.upload(X), c.m)
    Y = engine.download(dY)
    assert rc == 0 and engine.last_precond_sweep()["used"] and engine.last_precond_sweep()["pivots"] == 1
    want = np.stack(c.ref.xs[e], axis=1)
    close_enough("shifted_solve", kr.block_dist(Y, want), c.node_drift[e])
    assert engine.last_stats["krylov_iterations"] == c.ref.steps[e].max()


# ---- 2. factor accounting -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg3-N336-m16-r10", "csr-B-N333-m5-r30"])
def test_factor_accounting(engine, name):
    c = pc.case(name)
    setup(engine, c)
    np_ = len(c.pivots)
    first = run(engine, c)
    assert first[2]["factorizations"] == np_ == first[5]["factorizations"]
    assert first[5]["factor_bytes"] == np_ * engine.band_plan()[2]
    second = run(engine, c)
    assert second[2]["factorizations"] == 0 == second[5]["factorizations"] and second[5]["pivots"] == np_
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[3], second[3])
    engine.free_factors()
    third = run(engine, c)
    assert third[2]["factorizations"] == np_ and np.array_equal(first[0], third[0])


def test_a_direct_factor_of_the_same_shift_is_reused(engine):
    c = pc.case("cfg3-N336-m16-r10")
    setup(engine, c, precond=False)
    engine.set_solver("banded")
    engine.shifted_solve(c.pivots[0], engine.upload(c.Q), c.m)
    assert engine.last_stats["factorizations"] == 1
    setup(engine, c)
    got = run(engine, c)
    assert got[2]["factorizations"] == 0 and got[5]["factorizations"] == 0 and got[5]["used"]


# ---- 3. end to end --------------------------------------------------------------------------------------------------------
def test_feast_with_shift_preconditioner_equals_sparse_direct(engine):
    A, B, lam = fo.cfg3_problem(12, 10, 9)
    interval = (0.0, 0.5)
    inside = lam[(lam > interval[0]) & (lam < interval[1])]
    M0 = 2 * len(inside)
    direct = fk.feast(A, B, interval, M0=M0, engine=engine, solver="sparse_direct")
    pre = fk.feast(A, B, interval, M0=M0, engine=engine, solver="gmres", precond="shift")
    tol = 10.0 ** -int(fk.feastdefault(fk.feastinit())[3])
    assert direct.info == 0 and pre.info == 0 and pre.M == direct.M == len(inside)
    assert np.abs(np.sort(pre.lambda_) - np.sort(direct.lambda_)).max() <= tol * max(1.0, np.abs(direct.lambda_).max())
    for r in (pre, direct):
        # recomputed in fp64 on the host, in the suite's convention (test_gpu_feast.py); for these B-normalised vectors it is
        # below the driver's own |A x - lambda B x| / (max(|Emin|, |Emax|) |B x|), since |B x| <= 1.5 and the interval ends at 0.5
        res = np.linalg.norm(A @ r.q - (B @ r.q) * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
        print("precond feast: host residual %.3e, driver %.3e, loops %d" % (res.max(), r.res.max(), r.loop))
        assert res.max() <= tol, res.max()
    log = pre.stats["precond"]
    assert len(log) == pre.loop + 1
    assert log[0]["factorizations"] == 1 and all(l["factorizations"] == 0 for l in log[1:])
    assert all(l["used"] and not l["fell_back"] and len(l["pivots"]) == 1 and l["node_pivot"] == [0] * 8 for l in log)
    assert all(l["substitution_sweeps"] > 0 and max(l["lock_steps"]) > 0 for l in log)
    assert pre.stats["factorizations"] == 1
    # the handle still reports the last loop's sweep: the log's last entry says the same
    last = engine.last_precond_sweep()
    assert last["used"] and last["pivots"] == len(log[-1]["pivots"]) == 1
    for key in ("factorizations", "substitution_sweeps", "factor_bytes", "fell_back"):
        assert last[key] == log[-1][key], (key, last, log[-1])
    assert last["factor_bytes"] == engine.band_plan()[2]
    # the factors went with the call: the same call again factors its pivot again (a kept factor would be matched by shift)
    again = fk.feast(A, B, interval, M0=M0, engine=engine, solver="gmres", precond="shift")
    assert [l["factorizations"] for l in again.stats["precond"]] == [l["factorizations"] for l in log]
    assert again.stats["factorizations"] == 1 and np.allclose(again.lambda_, pre.lambda_, rtol=0.0, atol=tol)
    # ... and so did the setting
    setup(engine, pc.case("cfg3-N336-m16-r10"), precond=False)
    run(engine, pc.case("cfg3-N336-m16-r10"))
    assert not engine.last_precond_sweep()["used"]


def _circle(A, B, center, count):
    ev = sla.eigvals(A.toarray(), B.toarray())
    d = np.sort(np.abs(ev - center))
    radius = 0.5 * (d[count - 1] + d[count])
    return ev[np.abs(ev - center) < radius], radius


def test_feast_general_with_two_pivots(engine):
    A, B = gc.nonsymmetric_pair()
    center = 25.0 + 0.0j
    inside, radius = _circle(A, B, center, 6)
    r = fk.feast_general(A, B, center, radius, M0=12, engine=engine, solver="gmres", solver_restart=30, precond="shift",
                         precond_shifts=2)
    assert r.info == 0 and r.M == len(inside)
    key = lambda z: (round(z.real, 6), round(z.imag, 6))
    assert np.allclose(sorted(r.lambda_, key=key), sorted(inside, key=key), atol=1e-8)
    log = r.stats["precond"]
    assert log[0]["factorizations"] == 2 and all(l["factorizations"] == 0 for l in log[1:]) and len(set(log[0]["node_pivot"])) == 2


def test_explicit_off_contour_pivots(engine):
    A, B, lam = fo.cfg3_problem(8, 7, 6)
    interval = (0.0, 0.5)
    inside = lam[(lam > interval[0]) & (lam < interval[1])]
    piv = [0.1 + 0.3j, 0.4 + 0.3j]
    r = fk.feast(A, B, interval, M0=2 * len(inside), engine=engine, solver="gmres", precond="shift", precond_shifts=piv)
    assert r.info == 0 and r.M == len(inside) and np.allclose(np.sort(r.lambda_), inside, atol=1e-9)
    log = r.stats["precond"]
    assert log[0]["pivots"] == piv and log[0]["factorizations"] == 2
    Z, _ = pc.contour8(*interval)
    assert log[0]["node_pivot"] == [int(np.argmin([abs(z - p) for p in piv])) for z in Z]


# ---- 4. nothing else moved ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg3-N336-m16-r10", "ragged-nonsym-N323-m17-r8"])
def test_cleared_setting_leaves_the_plain_sweep_bitwise(name):
    """A GMRES sweep after feasthip_set_preconditioner(h, 0, ...) returns the bits of a fresh handle that never had one."""
    c = pc.case(name)
    outs = []
    for had in (False, True):
        eng = fk.HipEngine(0)
        try:
            setup(eng, c, True, maxit=40, precond=False)
            if had:
                eng.set_preconditioner(c.pivots, c.node_pivot)
                run(eng, c)
                eng.set_preconditioner(None)
            got = run(eng, c)
            assert not got[5]["used"] and got[5]["substitution_sweeps"] == 0
            outs.append(got)
        finally:
            eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][3], outs[1][3])
    assert outs[0][1] == outs[1][1] and outs[0][2]["spmm_calls"] == outs[1][2]["spmm_calls"]


def test_unpreconditioned_nodes_run_the_plain_operator(engine):
    """node_pivot = -1 for half the nodes: those run the plain GMRES sweep (restart 30 here: unpreconditioned GMRES(10) needs
    hundreds of steps on this pencil), the others the preconditioned one, and every node converges.  The plain nodes reach the
    same solutions by other iterates, so the sum agrees with the reference only as far as rtol = 1e-10 times the condition
    of the shifted matrices allows: their norm is below 12, the nearest eigenvalue at least 1e-2 away, hence 1e-6."""
    c = pc.case("cfg3-N336-m16-r10")
    setup(engine, c)
    engine.set_solver("gmres", rtol=pc.RTOL, atol=0.0, maxit=2000, restart=30)
    engine.set_preconditioner(c.pivots, [0, 0, 0, 0, -1, -1, -1, -1])
    out = run(engine, c)
    assert out[5]["used"] and out[5]["pivots"] == 1 and out[1] == [0] * 8
    dist = kr.block_dist(out[0], c.ref.out)
    print("precond mixed: distance %.3e" % dist)
    assert dist <= 1e-6


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_abi_refusals(engine):
    c = pc.case("cfg3-N336-m16-r10")
    setup(engine, c, precond=False)
    dQ = engine.upload(c.Q)

    def refused(match):
        with pytest.raises(fk.FeastHipError, match=match) as e:
            engine.contour_apply(dQ, c.m)
        assert e.value.code == 9
        with pytest.raises(fk.FeastHipError, match=match) as e:
            engine.shifted_solve(c.Z[0], dQ, c.m)
        assert e.value.code == 9

    with pytest.raises(fk.FeastHipError, match="count") as e:
        engine.set_preconditioner(c.pivots, [0] * 7)
    assert e.value.code == 9
    with pytest.raises(fk.FeastHipError, match="node_pivot") as e:
        engine.set_preconditioner(c.pivots, [1] * 8)
    assert e.value.code == 9
    with pytest.raises(fk.FeastHipError, match="imaginary") as e:
        engine.set_preconditioner([0.25], [0] * 8)
    assert e.value.code == 9
    engine.set_preconditioner(c.pivots, c.node_pivot)
    for solver in ("cocg", "bicgstab", "banded"):
        engine.set_solver(solver)
        refused("FEASTHIP_SOLVER_GMRES")
    engine.set_solver("gmres", factor_precision=32)
    refused("factor_precision = 32")
    engine.set_solver("gmres")
    engine.set_node_solver([4] + [0] * 7)
    refused("direct node")
    engine.set_node_solver(None)
    engine.set_adjoint(True)
    refused("adjoint")
    engine.set_adjoint(False)
    engine.set_problem(c.A.toarray(), c.B.toarray())
    engine.set_solver("gmres")
    refused("CSR problem")
    # another node count clears the setting: the dense GMRES sweep runs again
    engine.set_contour(c.Z[:4], c.W[:4], 2.0)
    engine.contour_apply(dQ, c.m)
    assert not engine.last_precond_sweep()["used"]


def test_operator_handle_is_refused(engine):
    c = pc.case("csr-I-N45-m7-r30")
    A = c.A.tocsr()
    engine.set_operator(c.N, lambda X: A @ X, None, real=True, symmetric=True)
    engine.set_contour(c.Z, c.W, 2.0)
    engine.set_solver("gmres")
    engine.set_preconditioner(c.pivots, c.node_pivot)
    try:
        with pytest.raises(fk.FeastHipError, match="CSR problem") as e:
            engine.contour_apply(engine.upload(c.Q), c.m)
        assert e.value.code == 9
    finally:
        engine.set_preconditioner(None)
        engine.set_problem(c.A, c.B)         # (the teardown's direct solver is refused while an operator is set)


@pytest.mark.parametrize("terms", [False, True], ids=["polynomial", "terms"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
def test_polynomial_and_term_handles_are_refused(engine, terms, sparse):
    """A polynomial handle and a term handle (dense or CSR coefficients): the sweep names the CSR pencil it needs, the
    single-shift solve names the handle; both FEASTHIP_ERROR_FPM."""
    c = pc.case("csr-I-N45-m7-r30")
    setup(engine, c, precond=False)
    coeffs = [c.A.tocsr(), sp.identity(c.N, format="csr")]
    try:
        if sparse:
            engine.set_polynomial_csr(*polynomial_union_csr(coeffs), terms=terms)
        else:
            engine.set_polynomial([m.toarray() for m in coeffs], terms=terms)
        engine.set_contour(c.Z, c.W, 2.0)
        engine.set_preconditioner(c.pivots, c.node_pivot)
        dQ = engine.upload(c.Q)
        with pytest.raises(fk.FeastHipError, match="set_preconditioner.*CSR problem.*polynomial handle") as e:
            engine.contour_apply(dQ, c.m)
        assert e.value.code == 9
        with pytest.raises(fk.FeastHipError, match="polynomial handle") as e:
            engine.shifted_solve(c.Z[0], dQ, c.m)
        assert e.value.code == 9
    finally:
        engine.set_preconditioner(None)
        engine.set_problem(c.A, c.B)


TWO_RANKS = r'''
import os, sys, time, faulthandler
faulthandler.dump_traceback_later(200, exit=True)
sys.path[:0] = [r"{root}", r"{root}/oracle", r"{root}/tests"]
import numpy as np
import feastkit_jl_amd as fk
import precond_cases as pc
rank, out = int(sys.argv[1]), r"{out}"
eng = fk.HipEngine(0)
uidf = os.path.join(out, "uid.bin")
if rank == 0:
    open(uidf + ".tmp", "wb").write(eng.comm_unique_id()); os.rename(uidf + ".tmp", uidf)
else:
    t0 = time.time()
    while not os.path.exists(uidf):
        time.sleep(0.01); assert time.time() - t0 < 60
eng.comm_init(2, rank, open(uidf, "rb").read(), "shm")
A, B = pc.CASES["csr-I-N45-m7-r30"][0]()
Z, W = pc.contour8(10.0, 20.0)
piv, node_pivot = pc.pivots_of("arcs:2", Z)
eng.set_problem(A, B); eng.set_contour(Z, W, 2.0); eng.set_node_range(4 * rank, 4)
eng.set_solver("gmres", rtol=1e-10, atol=0.0, maxit=200, restart=30)
eng.set_preconditioner(piv, node_pivot)
dQ = eng.upload(fk.seeded_subspace(45, 7))
# the same refusal on every rank, before the collective: nobody is left waiting
for call in (lambda: eng.contour_apply(dQ, 7), lambda: eng.shifted_solve(Z[0], dQ, 7)):
    try:
        call()
        raise SystemExit("not refused")
    except fk.FeastHipError as err:
        assert err.code == 9 and "more than one rank" in str(err) and "set_preconditioner" in str(err), str(err)
eng.set_preconditioner(None)
dP, status, st = eng.contour_apply(dQ, 7)          # cleared: the two-rank sweep is taken again (plain GMRES(30) on this
assert set(int(v) for v in status[:8]) <= {{0, 5}}   # dense spectrum converges on some nodes only: 0 or 5, never a refusal)
assert not eng.last_precond_sweep()["used"]
eng.barrier(); eng.comm_destroy(); eng.close()
print("rank", rank, "ok")
'''


def test_two_ranks_are_refused(tmp_path):
    """A communicator with two ranks (shared-device transport, two processes on one card): FEASTHIP_ERROR_FPM on both."""
    script = tmp_path / "two_ranks.py"
    script.write_text(TWO_RANKS.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", FEASTHIP_COMM_TIMEOUT_S="60")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs


@pytest.mark.parametrize("kw,match", [
    (dict(solver="cocg"), "solver='gmres'"), (dict(solver="sparse_direct"), "solver='gmres'"),
    (dict(solver="gmres", inner_precision=32), "inner_precision=64"), (dict(solver="gmres", group=object()), "group"),
    (dict(solver="gmres", direct_nodes=[0]), "direct_nodes"), (dict(solver="gmres", M0="auto"), "M0='auto'"),
    (dict(solver="gmres", precond_shifts=[0.3]), "imaginary"), (dict(solver="gmres", precond_shifts=0), "precond_shifts"),
    (dict(solver="gmres", precond="ilu"), "precond must be"),
])
def test_python_refusals(engine, kw, match):
    A, B, _ = fo.cfg3_problem(8, 7, 6)
    args = dict(M0=8, engine=engine, precond="shift")
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        fk.feast(A, B, (0.0, 0.5), **args)
    with pytest.raises(ValueError, match=match):
        fk.feast_general(A, B, 0.25 + 0.0j, 0.25, **args)


def test_python_refusals_of_input_and_mode(engine):
    A, B, _ = fo.cfg3_problem(8, 7, 6)
    with pytest.raises(ValueError, match="sparse input"):
        fk.feast(A.toarray(), B.toarray(), (0.0, 0.5), M0=8, engine=engine, solver="gmres", precond="shift")
    fpm = fk.feastinit()
    fpm[14] = 2
    with pytest.raises(ValueError, match="fpm\\[14\\]"):
        fk.feast(A, B, (0.0, 0.5), M0=8, fpm=fpm, engine=engine, solver="gmres", precond="shift")
    with pytest.raises(ValueError, match="two_sided.*sparse_direct"):
        fk.feast_general(A, B, 0.25 + 0.0j, 0.25, M0=8, engine=engine, solver="gmres", precond="shift", two_sided=True)
