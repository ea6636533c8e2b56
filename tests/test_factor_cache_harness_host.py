"""CPU sanitizer build of the factor caches' host-only rules (tests/host_factor_cache_harness.cpp over csrc/fh_factor_cache.hpp):
the reuse test, the stale / commit bookkeeping, the one-off slot and the slots matched by shift under AddressSanitizer +
UndefinedBehaviorSanitizer with leak detection, on counting malloc / free allocators."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_factor_cache_rules_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_factor_cache_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "host_factor_cache_harness.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-4000:]
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(run.stdout[-3000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("OK") and "FAIL" not in run.stdout, run.stdout[-4000:]
