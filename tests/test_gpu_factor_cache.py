"""GPU tests of the factor cache's reuse rule, slot by slot, on both direct solvers and all three sparse plans: a sweep factors
only the nodes whose shift is not held (none on the same contour, ONE after a single shift moved), a one-off shift equal to a
local node takes that node's slot and any other the extra slot, and with caching off everything is factored.  Each sweep is
checked against a host contour sum, so a slot that kept the factors of another shift would show."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import feastkit_jl_amd as fk

pytestmark = pytest.mark.gpu

NE, M0 = 4, 8
CENTER, RADIUS = 1.0, 0.5


def problem(kind):
    """(A, solver, environment, `blocked` of the plan, upper bound of the spectrum): symmetric A with eigenvalues in [0, bound], B = I"""
    if kind == "dense":                                   # N = 160: two 128-blocks, the second ragged
        n = 160
        return np.diag(2.0 * np.ones(n)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1), "direct", {}, None, 4.0
    if kind == "narrow":
        n = 200
        return sp.csr_matrix(sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])), "banded", {}, 0, 4.0
    g = 24                                                # five-point grid, N = 576 (a scaling per plan: the engine keeps resident matrices)
    T = sp.diags([-np.ones(g - 1), 2.0 * np.ones(g), -np.ones(g - 1)], [-1, 0, 1])
    L = sp.kron(sp.identity(g), T) + sp.kron(T, sp.identity(g))
    if kind == "band":
        return sp.csr_matrix(L * 0.999), "banded", {"FH_WBAND": "1", "FH_MF": "0"}, 1, 8.0
    return sp.csr_matrix(L), "banded", {"FH_MF": "1"}, 2, 8.0


def host_sweep(A, Z, W, Q):
    n = A.shape[0]
    if sp.issparse(A):
        return sum(2 * W[e] * spla.splu((Z[e] * sp.identity(n) - A).tocsc().astype(complex)).solve(Q.astype(complex)) for e in range(len(Z)))
    return sum(2 * W[e] * np.linalg.solve(Z[e] * np.eye(n) - A, Q) for e in range(len(Z)))


@pytest.mark.parametrize("kind", ["dense", "narrow", "band", "multifrontal"])
def test_sweeps_factor_only_the_slots_that_do_not_hold_their_shift(engine, monkeypatch, kind):
    A, solver, env, blocked, top = problem(kind)
    for name in ("FH_WBAND", "FH_MF"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    n = A.shape[0]
    engine.set_problem(A, None)
    engine.set_solver(solver)
    if blocked is not None:
        assert engine.band_plan()[3] == blocked
    fpm = fk.feastdefault(fk.feastinit()); fpm[2] = NE
    Z, W = fk.feast_contour(CENTER - RADIUS, CENTER + RADIUS, fpm)
    Z, W = np.asarray(Z), np.asarray(W)
    assert len(Z) == NE
    engine.set_real_projection(False)
    Q = fk.seeded_subspace(n, M0)
    dQ = engine.upload(Q)
    # z I - A is normal: cond = max |z - lambda| / min |z - lambda| <= (|z| + top) / |Im z|; LU with partial pivoting is backward
    # stable, so a solve is off by about n eps cond relative to the solution, and so is the weighted sum (10: slack for the
    # growth factor and the reference's own error)
    moved = Z.copy(); moved[2] += 0.01j
    cond = max((abs(z) + top) / abs(z.imag) for z in np.concatenate([Z, moved]))
    tol = 10 * n * np.finfo(float).eps * cond

    def sweep(contour, nfact):
        engine.set_contour(contour, W, 2.0)
        dP, status, st = engine.contour_apply(dQ, M0)
        got, want = engine.download(dP, M0), host_sweep(A, contour, W, Q)
        err = np.abs(got - want).max() / np.abs(want).max()
        print("%s: factorizations %d (expected %d), error %.2e (bound %.2e)" % (kind, st["factorizations"], nfact, err, tol))
        assert st["factorizations"] == nfact and not status[:NE].any() and err <= tol
        return got

    first = sweep(Z, NE)
    assert np.array_equal(sweep(Z, 0), first)             # the same contour: nothing is factored
    sweep(moved, 1)                                       # one shift moved: its slot alone
    back = sweep(Z, 1)                                    # and back: that slot again, the others still hold theirs
    # one-off shifts: a local node's shift takes the node's slot, another shift the extra slot, and neither evicts a node
    X = engine.upload(Q)
    for z, nfact in ((Z[1], 0), (0.9 + 0.3j, 1), (0.9 + 0.3j, 0), (0.8 + 0.3j, 1), (Z[3], 0)):
        _dY, rc = engine.shifted_solve(z, X, M0)
        assert rc == 0 and engine.last_stats["factorizations"] == nfact, (z, engine.last_stats["factorizations"], nfact)
    assert np.array_equal(sweep(Z, 0), back)
    engine.set_solver(solver, cache_factors=False)        # caching off: every node, every time
    try:
        sweep(Z, NE)
        sweep(Z, NE)
    finally:
        engine.set_solver(solver)
        engine.free_factors()
