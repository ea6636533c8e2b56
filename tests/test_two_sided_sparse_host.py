"""Two-sided FEAST on sparse input, the host half: the cases of tests/two_sided_sparse_cases.py meet the conditions their
circles were chosen under and the host restatement converges on them, and the keyword validation of
feast_general(A_sparse, ..., two_sided=True) accepts the sparse direct solver without touching a device."""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import two_sided_sparse_cases as sc
from feastkit_jl_amd.hip_backend import check_two_sided
from two_sided_reference import residuals


@pytest.mark.parametrize("params", sc.PARAMS, ids=sc.IDS)
def test_sparse_cases_and_restatement(params):
    case = sc.make_case(*params)
    ref = sc.reference_run(params)
    print("N %d centre %s radius %.3f k %d gap ratio %.2f loops %d epsout %.2e overlap min %.3f eps_hist %s" % (
        case["N"], case["center"], case["radius"], case["k"], case["gap_ratio"], ref["loop"], ref.get("epsout", np.inf),
        ref["overlap"].min(), ["%.1e" % e for e in ref["eps_hist"]]))
    assert case["gap_ratio"] >= sc.MIN_GAP_RATIO
    assert len(case["lam_in"]) == case["k"]
    assert ref["info"] == 0 and ref["loop"] <= 8 and ref["M"] == case["k"]
    Y = ref["Y"] / np.linalg.norm(ref["Y"], axis=0)
    rr, rl = residuals(case["Ad"].astype(complex), None if case["Bd"] is None else case["Bd"].astype(complex), ref["lam"], ref["X"], Y)
    print("res_R %.2e res_L %.2e" % (rr.max(), rl.max()))
    assert rr.max() <= 1e-10 and rl.max() <= 1e-10


@pytest.mark.parametrize("solver", ["direct", "lu", "sparse_direct", "banded"])
def test_sparse_direct_solvers_pass_validation(solver):
    check_two_sided(True, solver)


@pytest.mark.parametrize("kw,word", [(dict(solver="bicgstab"), "solver"), (dict(solver="krylov"), "solver"), (dict(solver="gmres"), "solver"),
                                     (dict(inner_precision=32), "inner_precision"), (dict(group=object()), "group"),
                                     (dict(solver="banded", inner_precision=32), "inner_precision"),
                                     (dict(solver="sparse_direct", group=object()), "group"),
                                     (dict(solver="sparse_direct", direct_nodes=[0]), "direct_nodes")])
def test_sparse_keyword_validation_is_host_only(kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    A = sp.diags([np.full(7, -1.0), np.arange(1.0, 9.0), np.full(7, -0.5)], [-1, 0, 1], format="csr")
    with pytest.raises(ValueError, match=word):
        fk.feast_general(A, None, 0.0, 1.0, M0=4, two_sided=True, **kw)


def test_dense_input_keeps_its_solver_rule():
    check_two_sided(False, "direct")
    for solver in ("banded", "sparse_direct", "bicgstab"):
        with pytest.raises(ValueError, match="solver"):
            check_two_sided(False, solver)


def test_narrow_band_under_the_default_solver_names_the_way_out(monkeypatch):
    """solver='direct' on a pattern inside the library's narrow band means the one-workgroup band LU, which has no adjoint form:
    refused on the host with both ways out named; the explicit sparse direct solver passes the validation for the same matrix
    (the engine is the first thing it asks for)."""
    class Reached(Exception):
        pass

    def no_engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(fk.api, "_engine", no_engine)
    A = sp.diags([np.full(39, -1.0), np.arange(1.0, 41.0), np.full(39, -0.5)], [-1, 0, 1], format="csr")
    with pytest.raises(ValueError, match="sparse_direct.*dense input"):
        fk.feast_general(A, None, 0.0, 1.0, M0=4, two_sided=True)
    for solver in ("sparse_direct", "banded"):
        with pytest.raises(Reached):
            fk.feast_general(A, None, 0.0, 1.0, M0=4, two_sided=True, solver=solver)


def test_wider_patterns_take_the_dense_window_under_the_default_solver(monkeypatch):
    """Beyond the narrow band solver='direct' expands the matrix (N <= 12 288) and needs no plan query: the route is decided
    on the host."""
    case = sc.make_case(*sc.PARAMS[2])
    A2, B2, solver, sub, eng = fk.api._two_sided_sparse_route(case["A"], case["B"], "direct", 8, None, 0)
    assert solver == "direct" and eng is None and not sp.issparse(A2) and not sp.issparse(B2)
    assert "dense" in sub["used"] and np.array_equal(A2, case["Ad"])
