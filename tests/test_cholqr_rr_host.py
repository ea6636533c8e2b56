"""The staged rank-revealing Cholesky-QR on the CPU: the numpy restatement (tests/cholqr_rr_reference.py) against scipy's
column-pivoted QR on the fixtures of tests/cholqr_rr_cases.py, and the C++ stage routine the kernel restates
(csrc/fh_cholqr.hpp: pivoted_stage) under AddressSanitizer + UndefinedBehaviorSanitizer against the same fixtures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cholqr_rr_cases as cs
import cholqr_rr_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 1), (301, 16), (333, 23), (517, 32), (700, 47), (1000, 64)]
CASES = [(kind, N, m, cplx) for kind in cs.KINDS for (N, m) in SHAPES for cplx in (False, True)]


def _case(kind, N, m, cplx):
    X, ref = cs.make_case(kind, N, m, cplx, 1000 + m)
    return X, ref, (3 * m if kind == "f" else 0)


def assert_matches_scipy(got_rank, got_perm, got_rdiag, X, ref, big):
    """same rank, same pivot order up to ties, |R_kk| within 1e-6 relative for pivots above the threshold"""
    rank, piv, rd, r11, thr = cs.assert_unambiguous(X, cs.SQRT_EPS, ref, big)
    assert got_rank == rank
    got_rdiag = np.asarray(got_rdiag, dtype=float)
    np.testing.assert_allclose(got_rdiag[:rank], rd[:rank], rtol=1e-6, atol=0.0)
    for k in range(rank):
        if got_perm[k] == piv[k]:
            continue
        # a different column is a tie: scipy's pivot at this step has an equal within the rounding of the comparison
        near = np.abs(rd[:rank] - rd[k]) <= 1e-6 * rd[k]
        assert near.sum() > 1 or np.allclose(X[:, got_perm[k]], X[:, piv[k]], rtol=0, atol=0), (k, got_perm[k], piv[k])


@pytest.mark.parametrize("kind,N,m,cplx", CASES)
def test_numpy_restatement_matches_scipy_pivoted_qr(kind, N, m, cplx):
    X, ref, big = _case(kind, N, m, cplx)
    out = rr.staged_qr(X, cs.SQRT_EPS, ref, big)
    assert not out["fell_back"]
    assert_matches_scipy(out["rank"], out["perm"], out["rdiag"], X, ref, big)
    Q = out["Q"]
    if out["rank"]:
        assert np.abs(Q.conj().T @ Q - np.eye(out["rank"])).max() < 1e-13


def test_numpy_restatement_edge_cases():
    X, _ = cs.make_case("zero", 300, 16, False, 1)
    out = rr.staged_qr(X, cs.SQRT_EPS)
    assert out["rank"] == 0 and not out["fell_back"]
    X, _ = cs.make_case("a", 300, 16, True, 2)
    X[7, 3] = np.nan
    assert rr.staged_qr(X, cs.SQRT_EPS)["fell_back"]
    # a panel graded down to 1e-10 with a rank_tol at the floor eps * N needs a third stage
    rng = np.random.default_rng(3)
    sv = np.concatenate([np.geomspace(1.0, 1e-10, 20), np.zeros(12)])
    X = (np.linalg.qr(rng.standard_normal((300, 32)))[0] * sv) @ np.linalg.qr(rng.standard_normal((32, 32)))[0].T
    rank, piv, rd, _, _ = cs.assert_unambiguous(X, 1e-15)
    out = rr.staged_qr(X, 1e-15)
    assert rank == 20 and out["rank"] == rank and out["stages"] >= 3
    np.testing.assert_allclose(out["rdiag"], rd[:rank], rtol=1e-4)
    assert list(out["perm"]) == list(piv[:rank])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_stage_routine_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_cholqr_rr_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
           os.path.join(ROOT, "tests", "host_cholqr_rr_harness.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-4000:]
    shapes = [(300, 1), (301, 16), (333, 23), (350, 32), (400, 64)]
    cases = [(kind, N, m, cplx) for kind in cs.KINDS + ("zero",) for (N, m) in shapes for cplx in (False, True)]
    src, dst = tmp_path / "panels.txt", tmp_path / "out.txt"
    with open(src, "w") as f:
        for kind, N, m, cplx in cases:
            X, ref, big = _case(kind, N, m, cplx)
            ld = 16 if m <= 16 else 32 if m <= 32 else 64
            f.write("%d %d %d %d %.17g %.17g %d\n" % (N, m, ld, int(cplx), cs.SQRT_EPS, ref, big))
            vals = X.T.ravel()
            f.write(" ".join(("%.17g %.17g" % (v.real, v.imag)) if cplx else "%.17g" % v.real for v in vals) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok %d" % len(cases)), run.stdout[-4000:]
    lines = open(dst).read().split("\n")
    for i, (kind, N, m, cplx) in enumerate(cases):
        rank, stages, fell = (int(v) for v in lines[3 * i].split())
        perm = [int(v) for v in lines[3 * i + 1].split()]
        rdiag = [float(v) for v in lines[3 * i + 2].split()]
        X, ref, big = _case(kind, N, m, cplx)
        assert fell == 0, (kind, N, m, cplx)
        assert_matches_scipy(rank, perm, rdiag, X, ref, big)
        # the two restatements agree with each other (not in the stage count: fixtures b and e end their leading block at
        # 1e-5, the edge of the window, where rounding decides which stage takes the last pivot)
        want = rr.staged_qr(X, cs.SQRT_EPS, ref, big)
        assert rank == want["rank"] and 1 <= stages <= rr.MAX_STAGES, (kind, N, m, cplx)
        np.testing.assert_allclose(rdiag, want["rdiag"], rtol=1e-6)
