"""The library's environment switches (csrc/fh_knobs.hpp) on the CPU: every accessor's default, parse convention, clamp and
read time through tests/host_knobs_harness.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (one child process per
case: a once-per-process switch shows its read time only inside one run), and two properties of the tree by text search:
nothing else in csrc/ reads the environment, and DESIGN.md's switch table names exactly the variables of the header."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feastkit.jl_amd", "csrc")
NAME = re.compile(r"\b(?:FH|FEASTHIP|FEASTKIT|FEAST_BENCH)_[A-Z0-9_]+\b")

# what the harness prints with nothing set (accessors that take the caller's default get the harness's marker values:
# prof_period 13, lu_kb 0, lu_chunks 7, gmres_budget_bytes 12345, mf_nodes_per_call 21, mf_max_multiplier 1e3)
DEFAULTS = {
    "FH_DEBUG_TIMING": "0", "FH_PROF_PERIOD": "13", "FH_PROF_NOPOOL": "0", "FH_REORDER": "1", "FH_SPMM_ROW": "1", "FH_LDS_SPMM": "0",
    "FH_COCG_FUSED": "1", "FH_NO_SUM_MODE": "0", "FH_NO_SHARED_START": "0", "FH_NO_LAZY_START": "0", "FH_CHECK_EVERY": "16",
    "FH_GMRES_BUDGET_MB": "12345", "FH_NO_CHOLQR": "0", "FH_CHOLQR_TWO_PASS": "0", "FH_SMALL_MATMUL_VALU": "0", "FH_DENSE_OP_VALU": "0",
    "FH_EIG_NO_LDS": "0", "FH_LU_KB": "0", "FH_LU_SOLVE_32": "0", "FH_LU_GEMM_STAGED": "0", "FH_LU_LOOKAHEAD": "1", "FH_LU_PANEL_LEGACY": "0",
    "FH_LU_RESERVE": "4", "FH_LU_CHUNKS": "7", "FH_LU_TRSM_SUBST": "0", "FH_LU_3M": "1", "FH_LU_BLOCKINV": "1", "FH_WBAND_BLOCKINV": "1",
    "FH_WBAND": "0", "FH_MF": "-1", "FH_MF_LEAF": "64", "FH_MF_STORE_SLACK": "1.25", "FH_MF_STREAMS": "1", "FH_MF_SIDE": "1",
    "FH_MF_NODES_PER_CALL": "21", "FH_MF_MAX_MULTIPLIER": "1000", "FEASTHIP_COMM_TRANSPORT": "(null)", "FEASTHIP_COMM_TIMEOUT_S": "120",
    "FEASTHIP_COMM_STAGING_MB": str(32 << 20), "FEASTHIP_RCCL_LIB": "(null)",
}


def header_names():
    return set(re.findall(r'"((?:FH|FEASTHIP)_[A-Z0-9_]+)"', open(os.path.join(CSRC, "fh_knobs.hpp")).read()))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("knobs") / "host_knobs_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "host_knobs_harness.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-4000:]

    def run(steps, env=None):
        """the (name, value) pairs the harness prints for `steps`, started with only `env` of the library's variables set"""
        clean = {k: v for k, v in os.environ.items() if not NAME.fullmatch(k)}
        clean.update(env or {}, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([str(exe)] + list(steps), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=clean)
        assert r.returncode == 0, r.stdout[-4000:]
        return [tuple(line.split(" ", 1)) for line in r.stdout.splitlines()]

    return run


def value(harness, name, setting):
    return harness([name], {name: setting})[0][1]


def test_harness_covers_every_switch_of_the_header(harness):
    listed = [n for (n,) in harness(["--list"])]
    assert len(listed) == len(set(listed)) and set(listed) == header_names() == set(DEFAULTS)


def test_unset_gives_the_documented_default(harness):
    assert dict(harness(sorted(DEFAULTS))) == DEFAULTS


def test_parse_conventions(harness):
    # off-kind: set and atoi == 0 switches it off; atoi("") == 0
    for name in ("FH_COCG_FUSED", "FH_LU_3M", "FH_SPMM_ROW", "FH_LU_BLOCKINV", "FH_WBAND_BLOCKINV", "FH_MF_SIDE"):
        assert [value(harness, name, s) for s in ("", "0", "1", "x")] == ["0", "0", "1", "0"], name
    # on-kind: set and atoi != 0 switches it on
    for name in ("FH_WBAND", "FH_LDS_SPMM"):
        assert [value(harness, name, s) for s in ("", "0", "1", "2")] == ["0", "0", "1", "1"], name
    # present-kind: any value switches it on
    for name in ("FH_NO_CHOLQR", "FH_CHOLQR_TWO_PASS", "FH_LU_SOLVE_32", "FH_NO_LAZY_START", "FH_NO_SHARED_START", "FH_NO_SUM_MODE",
                 "FH_LU_TRSM_SUBST", "FH_LU_GEMM_STAGED", "FH_DEBUG_TIMING", "FH_PROF_NOPOOL", "FH_SMALL_MATMUL_VALU",
                 "FH_DENSE_OP_VALU", "FH_EIG_NO_LDS"):
        assert [value(harness, name, s) for s in ("", "0", "1")] == ["1", "1", "1"], name
    # plain values and strings
    assert value(harness, "FH_MF", "0") == "0" and value(harness, "FH_MF", "1") == "1"
    assert value(harness, "FH_LU_LOOKAHEAD", "0") == "0" and value(harness, "FH_REORDER", "2") == "2"
    assert value(harness, "FH_LU_RESERVE", "0") == "0" and value(harness, "FH_LU_PANEL_LEGACY", "1") == "1"
    assert value(harness, "FH_MF_MAX_MULTIPLIER", "2.5e4") == "25000"
    assert value(harness, "FEASTHIP_COMM_TRANSPORT", "shm") == "shm" and value(harness, "FEASTHIP_RCCL_LIB", "/x/librccl.so") == "/x/librccl.so"


@pytest.mark.parametrize("name,setting,want", [
    ("FH_MF_LEAF", "1", "8"), ("FH_MF_LEAF", "128", "128"),
    ("FH_MF_STREAMS", "9", "4"), ("FH_MF_STREAMS", "0", "1"), ("FH_MF_STREAMS", "3", "3"),
    ("FH_LU_KB", "100", "96"), ("FH_LU_KB", "1", "32"), ("FH_LU_KB", "256", "256"),
    ("FH_MF_STORE_SLACK", "0.5", "1.25"), ("FH_MF_STORE_SLACK", "2", "2"),
    ("FH_CHECK_EVERY", "0", "1"), ("FH_CHECK_EVERY", "4", "4"),
    ("FH_PROF_PERIOD", "0", "1"), ("FH_PROF_PERIOD", "91", "91"),
    ("FH_GMRES_BUDGET_MB", "0", str(1 << 20)), ("FH_GMRES_BUDGET_MB", "3", str(3 << 20)),
    ("FH_MF_NODES_PER_CALL", "0", "1"), ("FH_MF_NODES_PER_CALL", "3", "3"), ("FH_MF_NODES_PER_CALL", "99", "21"),
    ("FH_LU_CHUNKS", "0", "1"), ("FH_LU_CHUNKS", "4", "4"),
    ("FEASTHIP_COMM_STAGING_MB", "0", str(1 << 20)), ("FEASTHIP_COMM_STAGING_MB", "8", str(8 << 20)),
    ("FEASTHIP_COMM_TIMEOUT_S", "0.1", "1"), ("FEASTHIP_COMM_TIMEOUT_S", "7.5", "7.5"),
])
def test_clamps(harness, name, setting, want):
    assert value(harness, name, setting) == want


@pytest.mark.parametrize("name,setting,before,after", [
    ("FH_NO_LAZY_START", "1", "0", "1"), ("FH_CHOLQR_TWO_PASS", "1", "0", "1"), ("FH_NO_CHOLQR", "1", "0", "1"),
    ("FH_NO_SHARED_START", "1", "0", "1"), ("FH_GMRES_BUDGET_MB", "2", "12345", str(2 << 20)), ("FH_WBAND", "1", "0", "1"),
    ("FH_MF", "1", "-1", "1"), ("FH_MF_LEAF", "16", "64", "16"), ("FH_MF_NODES_PER_CALL", "3", "21", "3"), ("FH_LU_KB", "64", "0", "64"),
    ("FH_LU_SOLVE_32", "1", "0", "1"), ("FH_LU_LOOKAHEAD", "0", "1", "0"), ("FH_LU_RESERVE", "2", "4", "2"), ("FH_LU_CHUNKS", "1", "7", "1"),
    ("FH_LU_TRSM_SUBST", "1", "0", "1"), ("FH_NO_SUM_MODE", "1", "0", "1"),
])
def test_per_call_switches_follow_the_environment(harness, name, setting, before, after):
    """every switch the GPU tests and tools set inside a live process (read per call, plan, factorisation or handle)"""
    got = harness([name, "%s=%s" % (name, setting), name, "-" + name, name])
    assert [v for _, v in got] == [before, after, before]


@pytest.mark.parametrize("name,setting,first", [
    ("FH_COCG_FUSED", "0", "1"), ("FH_LDS_SPMM", "1", "0"), ("FH_LU_3M", "0", "1"), ("FH_SPMM_ROW", "0", "1"), ("FH_REORDER", "2", "1"),
    ("FH_PROF_PERIOD", "1", "13"), ("FH_LU_BLOCKINV", "0", "1"), ("FH_WBAND_BLOCKINV", "0", "1"), ("FH_MF_SIDE", "0", "1"),
    ("FH_DENSE_OP_VALU", "1", "0"), ("FH_SMALL_MATMUL_VALU", "1", "0"), ("FH_EIG_NO_LDS", "1", "0"), ("FH_PROF_NOPOOL", "1", "0"),
])
def test_per_process_switches_keep_their_first_read(harness, name, setting, first):
    got = harness([name, "%s=%s" % (name, setting), name])
    assert [v for _, v in got] == [first, first]
    # ... and the first read is the environment's: the same setting from the start is seen
    assert value(harness, name, setting) != first


def test_only_the_header_reads_the_environment():
    users = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and not f.endswith((".o", ".so"))
             and "getenv" in open(os.path.join(CSRC, f), errors="replace").read()]
    assert users == ["fh_knobs.hpp"]


def test_design_table_names_the_header_switches():
    """the variable column of DESIGN.md's switch table, without the rows of the Python shim and of bench.py"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text.split("## 9. Environment switches", 1)[1]
    rows = [line for line in section.splitlines() if line.startswith("| `")]
    named = set()
    for row in rows:
        named.update(NAME.findall(row.split("|")[1]))
    python_side = {n for n in named if n.startswith(("FEASTKIT_", "FEAST_BENCH_")) or n == "FEASTHIP_LIB"}
    assert python_side == {"FEASTKIT_DIRECT_SWITCH", "FEASTKIT_DIRECT_FLOPS", "FEASTHIP_LIB", "FEAST_BENCH_CPU_WORKERS", "FEAST_BENCH_NOPROF"}
    assert named - python_side == header_names()
