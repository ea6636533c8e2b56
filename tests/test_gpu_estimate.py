"""Stochastic eigenvalue-count estimate (fpm[14] = 2) and M0 = "auto" on the MI355X: the device's Rademacher block
against the numpy restatement, every sample against host dense solves, unbiasedness against the closed-form spectrum of
a 3-D Laplacian pencil, the solver paths, two ranks on one card, the automatic M0 and a failing node."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
from feastkit_jl_amd import workloads
from test_estimate import rademacher

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260515


def _fpm(nodes=None, general=False):
    fpm = fk.feastinit()
    fpm[14] = 2
    if nodes is not None:
        fpm[8 if general else 2] = nodes
    return fpm


def _herm_filter(lam, Emin, Emax, fpm):
    """f(x) = Re sum_e 2 w_e / (z_e - x) of the half contour fpm describes."""
    Z, W = fk.feast_contour(Emin, Emax, fk.feastdefault(fpm.copy()))
    return np.real((2.0 * W[None, :] / (Z[None, :] - np.asarray(lam)[:, None])).sum(axis=1))


def _host_samples(A, B, V, Z, W, scale, real_part):
    """t_j = v_j^T rho v_j, rho = sum_e scale w_e (z_e B - A)^{-1} B (real part under the real projection), dense solves."""
    A = A.toarray() if sp.issparse(A) else np.asarray(A)
    Bm = np.eye(A.shape[0]) if B is None else (B.toarray() if sp.issparse(B) else np.asarray(B))
    R = np.zeros(V.shape, dtype=np.complex128)
    for z, w in zip(Z, W):
        R += scale * w * np.linalg.solve(z * Bm - A, Bm @ V)
    if real_part:
        R = R.real
    return (V * R).sum(axis=0)


@pytest.fixture(scope="module")
def lap10k():
    """3-D Laplacian pencil with ~10^4 unknowns and its closed-form spectrum."""
    A, B, lam = workloads.laplacian_3d_pencil(25, 20, 20)
    return A, B, lam


def _gap_end(lam, lo, hi):
    """a point in the widest gap between lam[k] and lam[k+1] for lo <= k < hi (k + 1 eigenvalues below it)."""
    k = lo + int(np.argmax(np.diff(lam[lo:hi + 1])))
    return 0.5 * (lam[k] + lam[k + 1]), k + 1


def test_random_block_matches_restatement(engine):
    A, B, _ = workloads.laplacian_3d_pencil(20, 15, 10)
    engine.set_problem(A, B)
    N = A.shape[0]
    for seed, m in ((SEED, 70), (2 ** 64 - 12345, 5)):
        V = engine.random_block(m, seed).cpu().numpy().T          # (m, N) tensor = column-major N x m
        assert V.shape == (N, m)
        assert np.all(V.imag == 0.0)
        rows = np.arange(1000, 2500)                              # a row range that does not start at 0
        assert np.array_equal(V.real[1000:2500], rademacher(seed, rows, np.arange(m)))
        assert np.array_equal(V.real, rademacher(seed, np.arange(N), np.arange(m)))


def test_samples_exact_dense_and_csr(engine):
    rng = np.random.default_rng(7)
    n = 300
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.linspace(-2.0, 6.0, n)) @ Q.T
    A = 0.5 * (A + A.T)
    C = rng.standard_normal((n, n)) / np.sqrt(n)
    B = np.eye(n) + 0.1 * (C @ C.T)
    Ac, Bc, _ = workloads.laplacian_3d_pencil(12, 10, 8)
    for (AA, BB, Emin, Emax, m) in ((A, B, 0.0, 0.5, 16), (Ac, Bc, 0.0, 0.5, 24), (A, None, 1.0, 1.6, 8)):
        fpm = _fpm()
        r = fk.feast(AA, BB, (Emin, Emax), M0=m, fpm=fpm, engine=engine, seed=SEED + 1)
        assert r.info == 0 and r.lambda_.size == 0 and r.q.shape == (AA.shape[0], 0)
        est = r.stats["estimate"]
        assert est["nodes"] == 3 and est["seed"] == SEED + 1 and est["solver"] in ("direct", "banded")
        V = rademacher(SEED + 1, np.arange(AA.shape[0]), np.arange(m))
        Z, W = fk.feast_contour(Emin, Emax, fpm)
        h = _host_samples(AA, BB, V, Z, W, 2.0, True)
        t = est["samples"]
        assert np.all(np.abs(t - h) <= 1e-9 * np.maximum(np.abs(h), 1.0)), np.abs(t - h).max()
        assert r.M == max(0, int(round(t.mean())))


@pytest.mark.parametrize("nodes", [3, 8])
def test_unbiased_against_closed_form(engine, lap10k, nodes):
    A, B, lam = lap10k
    Emax, _ = _gap_end(lam, 20, 40)
    fpm = _fpm(nodes)
    r = fk.feast(A, B, (0.0, Emax), M0=64, fpm=fpm, engine=engine)
    est = r.stats["estimate"]
    assert r.info == 0 and est["nodes"] == nodes and len(est["samples"]) == 64
    expect = _herm_filter(lam, 0.0, Emax, _fpm(nodes)).sum()
    assert abs(est["mean"] - expect) <= 4.0 * est["stderr"], (est["mean"], expect, est["stderr"])


def test_count_within_one(engine, lap10k):
    A, B, lam = lap10k
    Emin, k0 = _gap_end(lam, 2, 8)
    Emax, k1 = _gap_end(lam, 12, 20)
    fpm = _fpm(8)
    r = fk.feast(A, B, (Emin, Emax), M0=256, fpm=fpm, engine=engine)      # four 64-column panels
    est = r.stats["estimate"]
    assert r.info == 0 and len(est["samples"]) == 256
    assert abs(r.M - (k1 - k0)) <= 1, (est["mean"], est["stderr"], k1 - k0)


def test_count_general_disc(engine):
    A, delta = workloads.disc_spectrum_general(N=1024)
    center, radius = 3.0 + 2.0j, 3.0
    fpm = _fpm(general=True)
    r = fk.feast_general(A, None, center, radius, M0=64, fpm=fpm, engine=engine)
    est = r.stats["estimate"]
    assert r.info == 0 and est["nodes"] == 6 and np.iscomplexobj(est["samples"])
    Z, W = fk.feast_gcontour(center, radius, fpm)
    expect = np.real((W[None, :] / (Z[None, :] - delta[:, None])).sum(axis=1)).sum()
    assert abs(np.real(est["mean"]) - expect) <= 4.0 * est["stderr"], (est["mean"], expect, est["stderr"])
    assert r.M == max(0, int(round(np.real(est["mean"]))))


def test_solver_paths_agree_and_repeat_bitwise(engine, lap10k):
    A, B, lam = lap10k
    Emax, _ = _gap_end(lam, 20, 40)
    d = fk.feast(A, B, (0.0, Emax), M0=64, fpm=_fpm(), engine=engine).stats["estimate"]
    k = fk.feast(A, B, (0.0, Emax), M0=64, fpm=_fpm(), engine=engine, solver="cocg").stats["estimate"]
    k2 = fk.feast(A, B, (0.0, Emax), M0=64, fpm=_fpm(), engine=engine, solver="cocg").stats["estimate"]
    assert d["solver"] == "banded" and k["solver"] == "cocg" and k["solver_tol"] == 1e-8
    assert abs(k["mean"] - d["mean"]) <= 0.05, (k["mean"], d["mean"])
    assert np.array_equal(k["samples"], k2["samples"])
    d2 = fk.feast(A, B, (0.0, Emax), M0=64, fpm=_fpm(), engine=engine).stats["estimate"]
    assert np.array_equal(d["samples"], d2["samples"])


WORKER = r'''
import os, sys
sys.path[:0] = [r"{root}", r"{root}/tests"]
import numpy as np, torch, torch.distributed as dist
import feastkit_jl_amd as fk
from feastkit_jl_amd import workloads
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=rank, world_size=2)
A, B, lam = workloads.laplacian_3d_pencil(16, 12, 10)
out = []
for solver in ("direct", "cocg"):
    eng = fk.HipEngine(0)
    fpm = fk.feastinit(); fpm[14] = 2
    r = fk.feast(A, B, (0.0, 0.42), M0=80, fpm=fpm, engine=eng, solver=solver)
    out += [r.info] + list(r.stats["estimate"]["samples"])
    eng.close()
np.save(r"{out}/e%d.npy" % rank, np.array(out, dtype=float))
dist.barrier(); dist.destroy_process_group()
'''


def test_two_ranks_one_gpu_match_single_rank(engine, tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, port=port, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    e0, e1 = np.load(tmp_path / "e0.npy"), np.load(tmp_path / "e1.npy")
    assert np.array_equal(e0, e1)
    A, B, _ = workloads.laplacian_3d_pencil(16, 12, 10)
    for i, solver in enumerate(("direct", "cocg")):
        fpm = fk.feastinit(); fpm[14] = 2
        one = fk.feast(A, B, (0.0, 0.42), M0=80, fpm=fpm, engine=engine, solver=solver).stats["estimate"]["samples"]
        got = e0[i * 81: (i + 1) * 81]
        assert int(got[0]) == 0
        # direct solves: the ranks' factors are the single rank's, only the order of the node sums differs; the Krylov
        # sweep's dot products are blocked by the number of local nodes, so its iterates differ in the last bits
        tol = 1e-12 if solver == "direct" else 1e-7
        assert np.abs(got[1:] - one).max() <= tol * np.abs(one).max(), (solver, np.abs(got[1:] - one).max())


def test_auto_m0_finds_every_eigenvalue(engine):
    A, B, lam = workloads.laplacian_3d_pencil(20, 16, 12)
    Emin, k0 = _gap_end(lam, 3, 8)
    Emax, k1 = _gap_end(lam, 30, 40)
    inside = lam[k0:k1]
    fpm = fk.feastinit()
    r = fk.feast(A, B, (Emin, Emax), M0="auto", fpm=fpm, engine=engine)
    assert r.info == 0 and r.M == len(inside), (r.info, r.M, len(inside))
    assert np.abs(np.sort(r.lambda_) - inside).max() < 1e-10
    assert r.stats["M0_auto"] >= len(inside)
    est = r.stats["estimate"]
    assert r.stats["M0_auto"] == fk.api.auto_M0(est, A.shape[0]) and est["nodes"] == 3
    assert int(fpm[14]) == 0                                       # the caller's parameters are the solve's


def test_auto_m0_general(engine):
    A, delta = workloads.disc_spectrum_general(N=1024)
    center = 3.0 + 2.0j
    dist = np.sort(np.abs(delta - center))
    k = 20 + int(np.argmax(np.diff(dist[20:41])))              # the circle passes through the widest gap
    radius = 0.5 * (dist[k] + dist[k + 1])
    inside = np.abs(delta - center) < radius
    r = fk.feast_general(A, None, center, radius, M0="auto", engine=engine)
    assert r.info == 0 and r.M == int(inside.sum()) and r.stats["M0_auto"] >= r.M
    assert np.abs(np.sort_complex(r.lambda_) - np.sort_complex(delta[inside])).max() < 1e-8


def test_failing_node_gives_its_status_and_no_estimate(engine, lap10k):
    A, B, lam = lap10k
    r = fk.feast(A, B, (0.0, 0.3), M0=16, fpm=_fpm(), engine=engine, solver="cocg", solver_maxiter=2)
    assert r.info == 5 and r.M == 0 and r.stats["estimate"] is None
    r = fk.feast(A, B, (0.0, 0.3), M0="auto", engine=engine, solver="cocg", solver_maxiter=2)
    assert r.info == 5 and r.M == 0 and r.stats["estimate"] is None
