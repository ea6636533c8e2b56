"""CPU sanitizer build of the adjoint substitution's host restatement (tests/host_mf_adjoint_harness.cpp): the plan of
csrc/fh_mf.hpp executed on the CPU and walked conjugate-transposed in the order of the device code (U^H leaves first, L^H and
the fronts' row permutations root first) against the residual of (zB - A)^H x = b, and the conjugate-transposed CSR set of
csrc/fh_ingest.hpp (fh_adjoint_csr) against a dense transpose, under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_multifrontal_adjoint_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_mf_adjoint_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
           os.path.join(ROOT, "tests", "host_mf_adjoint_harness.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-4000:]
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(run.stdout[-6000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-4000:]
    assert "row interchanges 0 " in run.stdout and "FAIL" not in run.stdout
