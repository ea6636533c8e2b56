"""Per-node solver on the GPU (feasthip_set_node_solver, the drivers' ``direct_nodes`` keyword): a Krylov sweep whose chosen
quadrature nodes are solved by the sparse direct solver.  Sweep parity against a host contour sum, the factor cache's
book-keeping, moments, the estimate, argument errors, and the drivers at reduced and full size."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feast_oracle as fo
import feastkit_jl_amd as fk

from kat_util import cplx, load_kats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = 4          # FEASTHIP_SOLVER_BANDED
NE = 8


def fpm_with(**kw):
    fpm = fk.feastinit()
    for k, v in kw.items():
        fpm[int(k[1:])] = v
    return fpm


def rand_block(N, m, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((N, m)).astype(np.complex128))


@pytest.fixture(scope="module")
def cfg3_small():
    A, B, lam = fo.cfg3_problem(16, 12, 10)
    Zne, Wne = fo.feast_contour(0.0, 0.42, NE)
    Q = rand_block(A.shape[0], 20, 11)
    ref = np.zeros(Q.shape, complex)
    rhs = B @ Q
    for z, w in zip(Zne, Wne):
        ref += 2 * w * spla.splu(sp.csc_matrix(z * B - A)).solve(rhs)
    return A, B, lam, Zne, Wne, Q, ref


def _setup(engine, A, B, Zne, Wne, solver, real, **kw):
    engine.set_problem(A, B)
    engine.set_contour(Zne, Wne, 2.0)
    engine.set_real_projection(real)
    engine.set_node_range(0, len(Zne))
    # the strict run of test_cfg3_reduced_reference_mode_and_fast_mode: tol 1e-12, up to 3000 iterations
    engine.set_solver(solver, rtol=1e-12, atol=1e-12, maxit=3000, **kw)


def _kinds(nodes, ne=NE):
    k = np.zeros(ne, dtype=np.int32)
    k[list(nodes)] = DIRECT
    return k


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("mode", ["cocg", "cocg_noshared", "bicgstab"])
def test_sweep_parity_and_bookkeeping(engine, cfg3_small, mode, real):
    A, B, lam, Zne, Wne, Q, ref = cfg3_small
    want = ref.real if real else ref
    solver = "bicgstab" if mode == "bicgstab" else "cocg"
    if mode == "cocg_noshared":
        os.environ["FH_NO_SHARED_START"] = "1"
    try:
        engine.free_factors()
        _setup(engine, A, B, Zne, Wne, solver, real)
        m = Q.shape[1]
        dQ = engine.upload(Q)
        out = {}
        engine.set_node_solver(None)
        dP, status, st_a = engine.contour_apply(dQ, m)
        out["a"] = engine.download(dP)
        it_a = engine.last_node_iterations(NE).copy()
        assert (status[:NE] == 0).all() and st_a["factorizations"] == 0 and (it_a > 0).all()
        # (b) the two nodes nearest the real axis direct
        engine.set_node_solver(_kinds([0, NE - 1]))
        dP, status, st_b = engine.contour_apply(dQ, m)
        out["b"] = engine.download(dP)
        it_b = engine.last_node_iterations(NE).copy()
        assert (status[:NE] == 0).all()
        assert it_b[0] == 0 and it_b[NE - 1] == 0 and (it_b[1:NE - 1] == it_a[1:NE - 1]).all()
        assert st_b["factorizations"] == 2
        # nodes do not interact: the Krylov nodes iterate as in (a) from the same zero guess
        assert st_b["krylov_iterations"] == int(it_a[1:NE - 1].sum())
        assert st_a["krylov_iterations"] == int(it_a.sum())
        dP, status, st_b2 = engine.contour_apply(dQ, m)                       # same contour: the cache holds both factors
        assert st_b2["factorizations"] == 0
        assert np.array_equal(engine.download(dP), out["b"])
        Z2, W2 = fo.feast_contour(0.0, 0.42, NE, fpm18=60)                     # the contour moves under the direct nodes
        engine.set_contour(Z2, W2, 2.0)
        assert engine.contour_apply(dQ, m)[2]["factorizations"] == 2
        engine.set_contour(Zne, Wne, 2.0)
        # (c) every node direct through the per-node setting, (d) the direct solver alone
        engine.set_node_solver(_kinds(range(NE)))
        dP, status, st_c = engine.contour_apply(dQ, m)
        out["c"] = engine.download(dP)
        assert (status[:NE] == 0).all() and st_c["krylov_iterations"] == 0 and not engine.last_node_iterations(NE).any()
        engine.set_node_solver(None)
        engine.set_solver("banded", rtol=1e-12)
        dP, status, st_d = engine.contour_apply(dQ, m)
        out["d"] = engine.download(dP)
        scale = np.abs(want).max()
        for key, P in out.items():
            err = np.abs(P - want).max() / scale
            print(mode, real, key, "rel err %.3e" % err)
            # tolerance of test_contour_apply_matches_oracle_sum
            assert err <= 1e-10, (mode, real, key, err)
    finally:
        os.environ.pop("FH_NO_SHARED_START", None)
        engine.set_node_solver(None)
        engine.free_factors()


def test_resident_sweep_with_ritz_warm_start(engine, cfg3_small):
    """The resident entry points with a Ritz warm start: two direct nodes against none, and against the host sum."""
    A, B, lam, Zne, Wne, _Q, _ref = cfg3_small
    m = 24
    Q0 = rand_block(A.shape[0], m, 5)
    outs = {}
    try:
        for key, nodes in (("none", []), ("two", [0, NE - 1])):
            _setup(engine, A, B, Zne, Wne, "cocg", True)
            engine.set_node_solver(_kinds(nodes) if nodes else None)
            status, _st = engine.contour_apply_resident(engine.upload(Q0), m, None)
            rank, Sq, Aq = engine.rr_reduce_resident(m, 1e-8)
            w, V = sla.eigh(Aq, Sq)
            engine.rr_ritz_resident(rank, V, w, rank)
            X = engine.download(engine.export_resident(rank, which=0), rank)        # the Ritz block the next sweep starts from
            status, st = engine.contour_apply_resident(None, rank, w)
            assert (status[:NE] == 0).all()
            outs[key] = (engine.download(engine.export_resident(rank, which=1), rank), X, w, rank, st)
        P0, X0, w0, r0, st0 = outs["none"]
        P1, X1, w1, r1, st1 = outs["two"]
        assert r0 == r1 and st1["krylov_iterations"] < st0["krylov_iterations"]
        assert st1["factorizations"] == 0                 # the first resident sweep on this contour factored both nodes
        # both runs swept THEIR Ritz block: compare each with the host contour sum of that block
        for P, X in ((P0, X0), (P1, X1)):
            ref = np.zeros(X.shape, complex)
            rhs = B @ X
            for z, wt in zip(Zne, Wne):
                ref += 2 * wt * spla.splu(sp.csc_matrix(z * B - A)).solve(rhs)
            err = np.abs(P - ref.real).max() / np.abs(ref.real).max()
            print("resident rel err %.3e" % err)
            assert err <= 1e-10
    finally:
        engine.set_node_solver(None)
        engine.free_factors()


def test_moments_with_direct_nodes(engine, cfg3_small):
    A, B, lam, Zne, Wne, Q, _ref = cfg3_small
    m = Q.shape[1]
    try:
        res = {}
        for key, nodes in (("none", []), ("two", [0, NE - 1])):
            _setup(engine, A, B, Zne, Wne, "bicgstab", False)
            engine.set_node_solver(_kinds(nodes) if nodes else None)
            dP, status, st, zAq, zSq = engine.contour_apply(engine.upload(Q), m, None, want_moments=True)
            assert (status[:NE] == 0).all()
            res[key] = (zAq, zSq)
        for a, b in zip(res["none"], res["two"]):
            err = np.abs(a - b).max() / np.abs(a).max()
            print("moments rel diff %.3e" % err)
            assert err <= 1e-9            # atol of test_variant_b_moments_on_gpu against the oracle
    finally:
        engine.set_node_solver(None)
        engine.free_factors()


def test_argument_errors_leave_the_handle_usable(engine, cfg3_small):
    A, B, lam, Zne, Wne, Q, ref = cfg3_small
    m = Q.shape[1]
    dQ = engine.upload(Q)
    try:
        _setup(engine, A, B, Zne, Wne, "cocg", False)
        with pytest.raises(fk.FeastHipError, match="count") as e:
            engine.set_node_solver(np.zeros(NE + 1, dtype=np.int32))
        assert e.value.code == 9
        with pytest.raises(fk.FeastHipError, match="kind") as e:
            engine.set_node_solver(np.array([0, 3] + [0] * (NE - 2), dtype=np.int32))
        assert e.value.code == 9
        engine.set_node_solver(_kinds([0]))
        engine.set_solver("gmres", rtol=1e-12, atol=1e-12, maxit=200)
        with pytest.raises(fk.FeastHipError, match="GMRES") as e:
            engine.contour_apply(dQ, m)
        assert e.value.code == 9
        engine.set_solver("cocg", rtol=1e-12, atol=1e-12, maxit=3000, factor_precision=32)
        with pytest.raises(fk.FeastHipError, match="factor_precision") as e:
            engine.contour_apply(dQ, m)
        assert e.value.code == 9
        # a dense problem
        n = 40
        T = np.diag(2.0 * np.ones(n)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
        engine.set_problem(T, None)
        engine.set_contour(Zne, Wne, 2.0)
        engine.set_node_solver(_kinds([0]))
        engine.set_solver("bicgstab", rtol=1e-12, atol=1e-12, maxit=500)
        with pytest.raises(fk.FeastHipError, match="dense") as e:
            engine.contour_apply(engine.upload(rand_block(n, 4, 1)), 4)
        assert e.value.code == 9
        # another node count clears the kinds; the handle still works
        _setup(engine, A, B, Zne, Wne, "cocg", False)
        engine.set_node_solver(_kinds([0, NE - 1]))
        Z6, W6 = fo.feast_contour(0.0, 0.42, 6)
        engine.set_contour(Z6, W6, 2.0)
        _dP, status, st = engine.contour_apply(dQ, m)
        assert st["factorizations"] == 0 and (engine.last_node_iterations(6) > 0).all()
        engine.set_contour(Zne, Wne, 2.0)
        dP, status, st = engine.contour_apply(dQ, m)
        assert st["factorizations"] == 0
        assert np.abs(engine.download(dP) - ref).max() <= 1e-10 * np.abs(ref).max()
    finally:
        engine.set_node_solver(None)
        engine.free_factors()


def _check_reduced(r, A, B, inside, ref):
    # the bounds of test_cfg3_reduced_reference_mode_and_fast_mode
    assert r.info == 0 and r.M == len(inside) == ref.M
    assert np.allclose(np.sort(r.lambda_), inside, atol=1e-10)
    assert np.allclose(np.sort(r.lambda_), np.sort(ref.lam), atol=1e-10)
    assert r.epsout <= 1e-12
    res = np.linalg.norm(A @ r.q - (B @ r.q) * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
    assert res.max() <= 1e-10


def test_feast_driver_reduced_cfg3(engine):
    A, B, lam = fo.cfg3_problem(16, 12, 10)
    Emin, Emax = 0.0, 0.42
    inside = lam[(lam >= Emin) & (lam <= Emax)]
    M0 = len(inside) + 12
    ref = fo.feast_hermitian(A, B, Emin, Emax, M0, ne=8, real_projection=True)
    assert ref.info == 0
    base = fk.feast(A, B, (Emin, Emax), M0=M0, fpm=fpm_with(f2=8, f4=40), engine=engine, solver="cocg", warm_start=True,
                    inner_rtol=1e-2, solver_maxiter=100)
    assert "direct_nodes" not in base.stats
    for spec in ([0, 7], 2, "auto"):
        r = fk.feast(A, B, (Emin, Emax), M0=M0, fpm=fpm_with(f2=8, f4=40), engine=engine, solver="cocg", warm_start=True,
                     inner_rtol=1e-2, solver_maxiter=100, direct_nodes=spec)
        _check_reduced(r, A, B, inside, ref)
        log = r.stats["direct_nodes"]
        print(spec, [(e["nodes"], e["factorizations"]) for e in log], r.loop, r.stats["krylov_iterations"])
        assert len(log) == r.loop + 1 and [e["loop"] for e in log] == list(range(r.loop + 1))
        for e, its in zip(log, r.stats["node_iterations"]):
            assert len(its) == 8 and all(its[n] == 0 for n in e["nodes"])
        if isinstance(spec, list):
            assert all(e["nodes"] == [0, 7] for e in log) and log[0]["factorizations"] == 2
            assert all(e["factorizations"] == 0 for e in log[1:])
            assert r.stats["krylov_iterations"] < base.stats["krylov_iterations"]
        elif spec == 2:
            assert log[0]["nodes"] == [] and all(len(e["nodes"]) == 2 for e in log[1:])
        else:
            assert log[0]["nodes"] == [] and "t_iter" in log[0]          # the rule ran after the first loop
            for prev, nxt in zip(log, log[1:]):
                assert set(prev["nodes"]) <= set(nxt["nodes"])           # a node once chosen stays chosen


def test_feast_driver_complex_hermitian_bicgstab(engine):
    """The pencil of test_complex_hermitian_sparse_generalized_bicgstab, two direct nodes."""
    N = 400
    rng = np.random.default_rng(7)
    S = sp.random(N, N, density=4.0 / N, random_state=3, format="csr")
    S = S + 1j * sp.random(N, N, density=4.0 / N, random_state=4, format="csr")
    A = sp.csr_matrix(S + S.conj().T + sp.diags(np.linspace(1.0, 40.0, N)))
    T = sp.random(N, N, density=2.0 / N, random_state=5, format="csr") * (0.3 + 0.2j)
    B = sp.csr_matrix(T + T.conj().T + sp.diags(2.0 + rng.random(N)))
    import scipy.linalg as sla
    ev = sla.eigh(A.toarray(), B.toarray(), eigvals_only=True)
    lo, hi = ev[5] - 1e-3, ev[14] + 1e-3
    inside = ev[(ev >= lo) & (ev <= hi)]
    for spec in ([0, 7], 2, "auto"):
        r = fk.feast(A, B, (lo, hi), M0=len(inside) + 14, fpm=fpm_with(f2=8, f4=80), engine=engine, solver="bicgstab",
                     solver_tol=1e-13, solver_maxiter=3000, direct_nodes=spec)
        assert r.M == len(inside) and r.info == 0
        assert np.allclose(np.sort(r.lambda_), inside, atol=1e-9)
        res = np.linalg.norm(A @ r.q - (B @ r.q) * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
        assert res.max() <= 1e-10
        assert len(r.stats["direct_nodes"]) == r.loop + 1


def test_estimate_with_direct_nodes(engine, cfg3_small):
    """fpm[14] = 2 through feasthip_estimate_count: the Krylov solver with two direct nodes against the all-direct estimate."""
    A, B, lam, Zne, Wne, _Q, _ref = cfg3_small
    try:
        _setup(engine, A, B, Zne, Wne, "banded", True)
        d, status, _ = engine.estimate_count(32, 7)
        engine.free_factors()                                                 # the all-direct run cached every node's factor
        engine.set_solver("cocg", rtol=1e-8, atol=1e-8, maxit=3000)          # ESTIMATE_TOL of the drivers
        engine.set_node_solver(_kinds([0, NE - 1]))
        k, status, st = engine.estimate_count(32, 7)
        assert (status[:NE] == 0).all() and st["factorizations"] == 2
        its = engine.last_node_iterations(NE)
        assert its[0] == 0 and its[NE - 1] == 0 and (its[1:NE - 1] > 0).all()
        print("estimate: max sample diff %.3e, means %.6f %.6f" % (np.abs(k - d).max(), np.mean(k.real), np.mean(d.real)))
        # bound of test_solver_paths_agree_and_repeat_bitwise between the direct and the Krylov estimate
        assert abs(np.mean(k.real) - np.mean(d.real)) <= 0.05
    finally:
        engine.set_node_solver(None)
        engine.free_factors()


def test_cfg3_full_size_direct_nodes(engine):
    """cfg 3 at full size with the bench's settings (test_cfg3_bench_settings_full_size): the two near-axis nodes direct."""
    A, B, lam = fo.cfg3_problem(50, 40, 25)
    inside = lam[(lam >= 0.0) & (lam <= 0.1775)]
    kw = dict(M0=64, engine=engine, solver="cocg", warm_start=True, inner_rtol=3e-2, solver_maxiter=50)
    base = fk.feast(A, B, (0.0, 0.1775), fpm=fpm_with(f2=16, f18=4000), **kw)
    r = fk.feast(A, B, (0.0, 0.1775), fpm=fpm_with(f2=16, f18=4000), direct_nodes=[0, 15], **kw)
    for x in (base, r):
        assert x.info == 0 and x.M == 44 and x.epsout <= 1e-12
        assert np.abs(np.sort(x.lambda_) - inside).max() <= 1e-10
        res = np.linalg.norm(A @ x.q - (B @ x.q) * x.lambda_, axis=0) / np.maximum(np.abs(x.lambda_), 1.0)
        assert res.max() <= 1e-12 * 10
    G = r.q.conj().T @ (B @ r.q)
    d = np.sqrt(np.abs(np.diag(G)))
    assert np.abs(G / np.outer(d, d) - np.eye(44)).max() <= 1e-8
    print("full size: krylov iterations %d -> %d, loops %d -> %d" % (base.stats["krylov_iterations"], r.stats["krylov_iterations"],
                                                                      base.loop, r.loop))
    assert r.stats["krylov_iterations"] < base.stats["krylov_iterations"]
    assert r.stats["direct_nodes"][0]["factorizations"] == 2
    # the default call, where the contour policy moves the contour under the direct nodes
    ra = fk.feast(A, B, (0.0, 0.1775), M0=64, fpm=fpm_with(f2=16), engine=engine, direct_nodes="auto")
    assert ra.info == 0 and ra.M == 44 and ra.epsout <= 1e-12
    assert np.abs(np.sort(ra.lambda_) - inside).max() <= 1e-10
    res = np.linalg.norm(A @ ra.q - (B @ ra.q) * ra.lambda_, axis=0) / np.maximum(np.abs(ra.lambda_), 1.0)
    assert res.max() <= 1e-12 * 10
    assert ra.loop <= 12 and len(ra.stats["direct_nodes"]) == ra.loop + 1
    print("auto:", [(e["nodes"], e["factorizations"]) for e in ra.stats["direct_nodes"]])


def test_interior_interval_auto_krylov_path_only(engine, monkeypatch):
    """The interval of test_default_call_interior_interval_full_size (40 eigenvalues around 0.52, indefinite shifted systems)
    with the Krylov path alone and direct_nodes="auto": the bounds of that test."""
    monkeypatch.setenv("FEASTKIT_DIRECT_SWITCH", "0")
    A, B, lam = fo.cfg3_problem(50, 40, 25)
    i0 = int(np.searchsorted(lam, 0.5))
    lo, hi = 0.5 * (lam[i0 - 1] + lam[i0]), 0.5 * (lam[i0 + 39] + lam[i0 + 40])
    r = fk.feast(A, B, (lo, hi), M0=64, fpm=fpm_with(f2=16, f4=40), engine=engine, direct_nodes="auto")
    print("interior: info %d loops %d epsout %.2e" % (r.info, r.loop, r.epsout),
          [(e["nodes"], e["factorizations"]) for e in r.stats["direct_nodes"]], r.stats["solver_substitution"])
    assert r.info == 0 and r.M == 40 and np.abs(np.sort(r.lambda_) - lam[i0:i0 + 40]).max() <= 1e-10
    res = np.linalg.norm(A @ r.q - (B @ r.q) * r.lambda_, axis=0) / np.maximum(np.abs(r.lambda_), 1.0)
    assert res.max() <= 1e-11
    assert isinstance(r.stats["direct_nodes"], list) and len(r.stats["direct_nodes"]) >= 1
    assert "fallback" not in r.stats["solver_substitution"]


def test_feast_general_sparse_with_direct_nodes(engine):
    """The MPI complex-general fixture of test_mpi_complex_general_fixture_on_csr through BiCGStab with direct nodes."""
    k = load_kats()["mpi_complex_general_diag4"]
    d = np.array([cplx(v) for v in k["diag"]])
    A = sp.diags(d).tocsr()
    B = sp.identity(len(d), dtype=np.complex128, format="csr")
    ckey = lambda x: (round(x.real, 8), round(x.imag, 8))
    want = [cplx(v) for v in k["expect_lambda"]]
    fp = dict(f3=k["fpm3"], f4=k["fpm4"], f8=k["fpm8"])
    for spec in ([0, k["fpm8"] - 1], 2, "auto"):
        r = fk.feast_general(A, B, cplx(k["center"]), k["radius"], M0=len(d), fpm=fpm_with(**fp), engine=engine,
                             solver="bicgstab", solver_maxiter=400, direct_nodes=spec)
        assert r.info == 0 and r.M == len(want), (spec, r.info, r.M)
        assert np.allclose(sorted(r.lambda_, key=ckey), sorted(want, key=ckey), atol=k["atol"]), spec
        log = r.stats["direct_nodes"]
        assert len(log) == r.loop + 1
        if isinstance(spec, list):
            assert all(e["nodes"] == spec for e in log) and log[0]["factorizations"] == 2
            assert all(e["factorizations"] == 0 for e in log[1:])
    # the default solver resolves to a direct solver outright here (narrow band): the keyword is ignored, and says so
    r = fk.feast_general(A, B, cplx(k["center"]), k["radius"], M0=len(d), fpm=fpm_with(**fp), engine=engine, direct_nodes=[0])
    assert r.info == 0 and r.stats["direct_nodes"] == {"ignored": "direct solver in force"}


def test_complex_symmetric_sparse_with_direct_nodes(engine):
    """The pencil of test_complex_symmetric_sparse_bicgstab (tests/test_gpu_feast.py), its bounds, with direct nodes."""
    n = 300
    rng = np.random.default_rng(2)
    diag = np.linspace(4.5, 8.0, n) + 0.3j * rng.uniform(-1, 1, n)
    idx = np.arange(10) * 29 + 5
    diag[idx] = 2.7 + 0.15 * rng.uniform(-1, 1, 10) + 0.1j * rng.uniform(-1, 1, 10)
    A = sp.diags([-0.2 * np.ones(n - 1), diag, -0.2 * np.ones(n - 1)], [-1, 0, 1], format="csr").astype(complex)
    ev = np.linalg.eigvals(A.toarray())
    c, r = 2.7 + 0.0j, 0.9
    inside = ev[np.abs(ev - c) <= r]
    key = lambda x: (round(x.real, 6), round(x.imag, 6))
    for spec in ([0, 15], 3, "auto"):
        fpm = fk.feastinit(); fpm[8] = 16; fpm[3] = 10; fpm[4] = 25
        try:
            got = fk.feast_hip_complex_symmetric(engine, A, None, c, r, 16, fpm, solver="bicgstab", solver_tol=1e-12,
                                                 solver_maxiter=3000, direct_nodes=spec)
        finally:
            engine.free_factors()
        assert got.info == 0 and got.M == len(inside) == 10
        assert np.allclose(sorted(got.lambda_, key=key), sorted(inside, key=key), atol=1e-8)
        assert got.epsout <= 1e-10
        log = got.stats["direct_nodes"]
        assert len(log) == got.loop + 1
        if isinstance(spec, list):
            assert log[0]["factorizations"] == 2 and all(e["nodes"] == [0, 15] for e in log)


RANK_WORKER = r'''
import json, os, sys
sys.path[:0] = [r"{root}", r"{root}/oracle", r"{root}/tests"]
import numpy as np, torch, torch.distributed as dist
import feast_oracle as fo, feastkit_jl_amd as fk
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=rank, world_size=2)
A, B, lam = fo.cfg3_problem(16, 12, 10)
out = {{}}
for name, spec in (("list", [0, 15]), ("auto", "auto")):
    eng = fk.HipEngine(0)
    fpm = fk.feastinit(); fpm[2] = 16; fpm[4] = 40
    r = fk.feast_hip_hermitian(eng, A, B, 0.0, 0.42, 32, fpm, solver="cocg", warm_start=True, inner_rtol=1e-2,
                               solver_maxiter=100, real_projection=True, direct_nodes=spec)
    log = [dict(e, **{{k: repr(v) for k, v in e.items() if isinstance(v, float)}}) for e in r.stats["direct_nodes"]]
    out[name] = {{"info": int(r.info), "M": int(r.M), "epsout": float(r.epsout), "loop": int(r.loop),
                 "lam": [float(v) for v in np.sort(r.lambda_)], "log": log, "local_nodes": r.stats["local_nodes"],
                 "node_iterations": r.stats["node_iterations"][0]}}
    eng.free_factors(); eng.close()
json.dump(out, open(r"{out}/n%d.json" % rank, "w"))
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_one_gpu_direct_nodes(engine, tmp_path):
    """Two node groups on one card (pattern of tests/test_gpu_multirank.py): direct_nodes=[0, 15] puts one direct node on each
    rank; the result equals the one-rank result, and both ranks report the same stats["direct_nodes"] -- also under "auto",
    whose times (floats, compared by repr) must be derived identically on every rank."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(RANK_WORKER.format(root=ROOT, port=port, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    g0, g1 = (json.load(open(tmp_path / ("n%d.json" % r))) for r in range(2))
    A, B, lam = fo.cfg3_problem(16, 12, 10)
    inside = lam[(lam >= 0) & (lam <= 0.42)]
    n = len(inside)
    for name, spec in (("list", [0, 15]), ("auto", "auto")):
        a, b = g0[name], g1[name]
        print(name, a["log"])
        assert a["log"] == b["log"] and len(a["log"]) == a["loop"] + 1
        assert a["lam"] == b["lam"] and (a["info"], a["M"], a["loop"]) == (b["info"], b["M"], b["loop"])
        assert set(a["local_nodes"]) | set(b["local_nodes"]) == set(range(16)) and not set(a["local_nodes"]) & set(b["local_nodes"])
        fpm = fk.feastinit(); fpm[2] = 16; fpm[4] = 40
        one = fk.feast_hip_hermitian(engine, A, B, 0.0, 0.42, 32, fpm, solver="cocg", warm_start=True, inner_rtol=1e-2,
                                     solver_maxiter=100, real_projection=True, direct_nodes=spec)
        engine.free_factors()
        assert (a["info"], a["M"]) == (0, n) == (one.info, one.M) and a["epsout"] <= 1e-12
        assert np.allclose(a["lam"], inside, atol=1e-10) and np.allclose(a["lam"], np.sort(one.lambda_), atol=1e-10)
    lst = g0["list"]
    assert all(e["nodes"] == [0, 15] for e in lst["log"]) and lst["log"][0]["factorizations"] == 2      # one on each rank, summed
    assert all(e["factorizations"] == 0 for e in lst["log"][1:])
    for g in (g0, g1):                        # each rank holds one of the two direct nodes, and it did not iterate
        its = dict(zip(g["list"]["local_nodes"], g["list"]["node_iterations"]))
        assert len({0, 15} & set(its)) == 1 and all(its[e] == 0 for e in {0, 15} & set(its))
        assert all(v > 0 for e, v in its.items() if e not in (0, 15))
