"""Per-node solver (feasthip_set_node_solver, the drivers' ``direct_nodes`` keyword), host side: the C ABI entries, the
selection rule feasthip_policy_pick_direct_nodes against its numpy restatement, and the keyword's validation, which runs
before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
from node_solver_reference import DIRECT, pick_direct_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pick(iters, max_direct, t_iter, t_solve, t_factor, loops_left):
    lib = fk.load_library()
    it = np.ascontiguousarray(iters, dtype=np.int32)
    kinds = np.full(len(it), -1, dtype=np.int32)
    k = lib.feasthip_policy_pick_direct_nodes(it.ctypes.data_as(ctypes.c_void_p), len(it), int(max_direct), float(t_iter),
                                              float(t_solve), float(t_factor), int(loops_left),
                                              kinds.ctypes.data_as(ctypes.c_void_p))
    return k, kinds


def test_node_solver_symbols_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "feasthip.h")).read(), flags=re.S)
    lib = fk.load_library()
    for name in ("feasthip_set_node_solver", "feasthip_policy_pick_direct_nodes", "feasthip_direct_plan_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in fk.SYMBOLS
        assert hasattr(lib, name)
    # a null handle is rejected without a device
    assert lib.feasthip_set_node_solver(None, 0, None) == 7
    assert lib.feasthip_direct_plan_bytes(None, 1, None, None) == 7


def test_pick_rule_equals_numpy_restatement():
    rng = np.random.default_rng(20261016)
    for _ in range(4000):
        ne = int(rng.integers(2, 57))
        iters = rng.integers(0, 500, ne) if rng.random() < 0.7 else rng.integers(40, 60, ne)      # the second kind has ties
        max_direct = int(rng.integers(0, ne + 1))
        t_iter, t_solve, t_factor = (float(10.0 ** rng.uniform(-6, -2)) for _ in range(3))
        loops_left = int(rng.integers(0, 20))
        k, kinds = _pick(iters, max_direct, t_iter, t_solve, t_factor, loops_left)
        k_ref, kinds_ref = pick_direct_nodes(iters, max_direct, t_iter, t_solve, t_factor, loops_left)
        assert k == k_ref and (kinds == kinds_ref).all(), (iters, max_direct, t_iter, t_solve, t_factor, loops_left)
        assert k <= max_direct and (kinds == DIRECT).sum() == k


def test_pick_rule_fixed_cases():
    # flat iterations: nothing beats the pure Krylov sweep
    k, kinds = _pick([55] * 16, 16, 1e-4, 1e-3, 5e-3, 4)
    assert k == 0 and not kinds.any()
    # the two near-axis nodes of cfg 3 and a cheap substitution: exactly those two
    iters = [170] + [49 + (i % 11) for i in range(14)] + [391]
    assert min(iters[1:15]) == 49 and max(iters[1:15]) == 59
    k, kinds = _pick(iters, 16, 1e-4, 4e-4, 1e-3, 5)
    assert k == 2 and list(np.nonzero(kinds)[0]) == [0, 15] and (kinds[[0, 15]] == DIRECT).all()
    # ties go to the lower index
    k, kinds = _pick([300, 50, 300, 50], 1, 1e-4, 1e-9, 0.0, 1)
    assert k == 0                                      # one of two equal maxima gone: the chain is as long as before
    k, kinds = _pick([300, 50, 300, 200], 3, 1e-4, 1e-6, 0.0, 1)
    assert k == 3 and list(np.nonzero(kinds)[0]) == [0, 2, 3]
    k, kinds = _pick([50, 300, 300, 300], 2, 1e-4, 1e-6, 0.0, 1)
    assert k == 0
    k, kinds = _pick([10, 300, 300, 20], 2, 1e-4, 1e-6, 0.0, 1)
    assert k == 2 and list(np.nonzero(kinds)[0]) == [1, 2]
    k, kinds = _pick([300, 300, 300, 20], 2, 1e-4, -1e-3, 0.0, 1)        # (a negative cost makes every k pay: lower indices first)
    assert k == 2 and list(np.nonzero(kinds)[0]) == [0, 1]
    # max_direct = 0 gives none
    k, kinds = _pick(iters, 0, 1e-4, 1e-6, 0.0, 5)
    assert k == 0 and not kinds.any()


def test_direct_nodes_keyword_is_validated_before_any_device_work():
    A = sp.diags([np.full(39, -1.0), np.full(40, 2.0), np.full(39, -1.0)], [-1, 0, 1], format="csr")
    fpm = fk.feastinit()
    fpm[2] = 8
    with pytest.raises(ValueError, match="sparse"):
        fk.feast(A.toarray(), None, (0.0, 1.0), M0=6, fpm=fpm, direct_nodes=[0])
    with pytest.raises(ValueError, match="gmres"):
        fk.feast(A, None, (0.0, 1.0), M0=6, fpm=fpm, solver="gmres", direct_nodes=[0])
    for bad in ([8], [-1], [0, 99]):
        with pytest.raises(ValueError, match="0..7"):
            fk.feast(A, None, (0.0, 1.0), M0=6, fpm=fpm, solver="cocg", direct_nodes=bad)
    for bad in (1.5, "some", [0.5], True, {"a": 1}):
        with pytest.raises(ValueError, match="direct_nodes"):
            fk.feast(A, None, (0.0, 1.0), M0=6, fpm=fpm, solver="cocg", direct_nodes=bad)
    with pytest.raises(ValueError, match="gmres"):
        fk.feast_general(A, None, 0.5, 0.5, M0=6, solver="gmres", direct_nodes=[0])
    with pytest.raises(ValueError, match="sparse"):
        fk.feast_general(A.toarray(), None, 0.5, 0.5, M0=6, direct_nodes="auto")
