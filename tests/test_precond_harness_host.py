"""CPU sanitizer build of the shift preconditioner's host-only rules (tests/host_precond_harness.cpp over csrc/fh_precond.hpp):
the arc rule and the nearest-pivot map under AddressSanitizer + UndefinedBehaviorSanitizer, and the plans it prints against the
Python driver's (hip_backend.precond_plan) and the reference's (precond_reference.arc_pivots)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import precond_reference as pr
from feastkit_jl_amd.hip_backend import precond_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pivot_rules_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_precond_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "host_precond_harness.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-4000:]
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(run.stdout[-3000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("OK") and "FAIL" not in run.stdout, run.stdout[-4000:]
    plans = re.findall(r"arcs ne=(\d+) k=(\d+) pivots([ \d]+) map([ \d]+)", run.stdout)
    assert len(plans) == 12
    for ne, k, pivots, nmap in plans:
        ne, k = int(ne), int(k)
        pivots, nmap = [int(v) for v in pivots.split()], [int(v) for v in nmap.split()]
        assert pr.arc_pivots(ne, k) == (nmap, pivots)
        Z = np.exp(1j * np.pi * (np.arange(ne) + 0.5) / ne)
        shifts, node_pivot = precond_plan(Z, k)
        assert node_pivot == nmap and shifts == [complex(Z[p]) for p in pivots]
