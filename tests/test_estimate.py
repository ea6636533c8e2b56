"""Stochastic eigenvalue-count estimate (fpm[14] = 2), host side: the estimate's parameter defaults, the C ABI entries,
and the numpy restatement of the device's Rademacher generator (csrc/fh_estimate.hip) that the GPU tests compare
against bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import feastkit_jl_amd as fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rademacher(seed, rows, cols):
    """v[i, j] for the given global row and column indices: +-1 from two rounds of the splitmix64 finaliser over
    (seed, row, column), mod 2^64 throughout."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    cols = np.asarray(cols, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (rows + np.uint64(1)))
        b = _mix64(key ^ (np.uint64(0xD1B54A32D192ED03) * (cols + np.uint64(1))))
    return np.where((b >> np.uint64(63)) != 0, -1.0, 1.0)


def test_feastdefault_estimate_defaults():
    fpm = fk.feastinit()
    fpm[14] = 2
    fk.feastdefault(fpm)
    assert (fpm[2], fpm[8], fpm[15]) == (3, 6, 1)
    # zero counts as unset, as for every other node count
    fpm = fk.feastinit()
    fpm[14], fpm[2], fpm[8] = 2, 0, 0
    fk.feastdefault(fpm)
    assert (fpm[2], fpm[8]) == (3, 6)


def test_feastdefault_estimate_keeps_caller_values():
    fpm = fk.feastinit()
    fpm[14], fpm[2], fpm[8], fpm[15] = 2, 8, 12, 2
    fk.feastdefault(fpm)
    assert (fpm[2], fpm[8], fpm[15]) == (8, 12, 1)     # fpm[15] = 1 always: right contour only


@pytest.mark.parametrize("v14", [0, 1])
def test_feastdefault_other_modes_unchanged(v14):
    fresh = fk.feastdefault(fk.feastinit())
    fpm = fk.feastinit()
    fpm[14] = v14
    fk.feastdefault(fpm)
    expect = fresh.copy()
    expect[14] = v14
    assert np.array_equal(fpm, expect)
    assert (fpm[2], fpm[8], fpm[15]) == (8, 16, 0)


def test_feastdefault_rejects_bad_mode():
    fpm = fk.feastinit()
    fpm[14] = 3
    with pytest.raises(ValueError, match=r"fpm\[14\]"):
        fk.feastdefault(fpm)


def test_estimate_symbols_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "feasthip.h")).read(), flags=re.S)
    lib = fk.load_library()
    for name in ("feasthip_estimate_count", "feasthip_random_block_dev"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in fk.SYMBOLS
        assert hasattr(lib, name)
    # a null handle is rejected without a device
    assert lib.feasthip_estimate_count(None, 4, 1, None, None, None) == 7
    assert lib.feasthip_random_block_dev(None, 4, 1, None) == 7


def test_auto_m0_rule():
    from feastkit_jl_amd.api import auto_M0
    assert auto_M0({"mean": 30.2, "stderr": 0.5}, 10_000) == 47          # ceil(1.5 * 31.2)
    assert auto_M0({"mean": 0.3, "stderr": 0.1}, 10_000) == 8            # at least 8
    assert auto_M0({"mean": 900.0, "stderr": 10.0}, 1000) == 1000        # at most N
    assert auto_M0({"mean": complex(4.0, 0.3), "stderr": 0.5}, 100) == 8


def test_bad_m0_string_is_rejected_before_any_device_work():
    with pytest.raises(ValueError, match="auto"):
        fk.feast(np.eye(4), None, (0.0, 1.0), M0="tight")
    with pytest.raises(ValueError, match="auto"):
        fk.feast_general(np.eye(4), None, 0.0, 1.0, M0="tight")


def test_rademacher_restatement_statistics():
    V = rademacher(20260515, np.arange(20000), np.arange(64))
    assert set(np.unique(V)) == {-1.0, 1.0}
    assert abs(V.mean()) < 0.01                                  # 1.28e6 entries: sd of the mean ~ 9e-4
    assert np.all(np.abs(V.mean(axis=0)) < 0.05)                 # per column: sd ~ 7e-3
    # columns are uncorrelated: the Gram matrix is ~ N I
    G = V.T @ V / V.shape[0]
    assert np.abs(G - np.eye(64)).max() < 0.05
    # another seed gives another block
    W = rademacher(20260516, np.arange(20000), np.arange(64))
    assert np.mean(V == W) < 0.55


def test_rademacher_restatement_does_not_depend_on_row_tiling():
    seed, rows, cols = 987654321, np.arange(7001), np.arange(70)
    whole = rademacher(seed, rows, cols)
    for tile in (1, 64, 1000, 4096):
        parts = [rademacher(seed, rows[r:r + tile], cols) for r in range(0, len(rows), tile)]
        assert np.array_equal(np.vstack(parts), whole)
    # nor on the column tiling (panels of 64)
    assert np.array_equal(np.hstack([rademacher(seed, rows, cols[:64]), rademacher(seed, rows, cols[64:])]), whole)
    # a row range that does not start at 0 is the corresponding slice
    assert np.array_equal(rademacher(seed, np.arange(1234, 2345), cols), whole[1234:2345])
