"""The shifted COCG restatement (shifted_krylov_reference.py) against krylov_reference's per-node five-launch COCG
(cocg5) in np.clongdouble: in exact arithmetic every node of the family walks through the iterates of its own COCG solve.
Standard problems only (B = None, real A: shifted_cases.PROBLEMS), all 16 nodes of the half contour, from the zero guess
and from the collinear Ritz warm start; iterates of every node after k steps (maxit = k, rtol = 1e-14) and the
per-(node, column) step counts of inexact solves.  No GPU.

The bound is measured, not chosen: D = the distance of per-node cocg5 in complex128, its dots summed over kr.DRIFT_ORDERS'
permuted chunks, from cocg5 in long double, the largest over the nodes and columns of the case at step k (the family is
ONE recurrence: the rounding of the seed reaches every node, so the case, not the single node, is the unit); a node's
shifted iterate must lie within kr.tolerance(D) = max(32 D, 64 eps) of its long-double cocg5 iterate.  Measured here
(k <= 33, zero guess / warm start):

    lap-N336    D <= 3.0e-11 / 2.5e-11   long-double shifted <= 5.2e-13 / 5.4e-14   complex128 shifted <= 6.3e-10 / 7.6e-11
    lap-N1080   D <= 5.7e-12 / 3.3e-13   long-double shifted <= 5.9e-14 / 7.3e-16   complex128 shifted <= 1.5e-10 / 9.5e-13
    rand-N45    D <= 3.8e-08 / 2.6e-07   long-double shifted <= 3.6e-09 / 6.9e-10   complex128 shifted <= 3.0e-06 / 9.2e-06

(the complex128 column is printed, not asserted: it is what the device computes in, and test_gpu_shifted_cocg.py holds the
device to the restatement's own fp64 drift).  Against a node's OWN D the long-double shifted iterate uses at most 0.23 of
32 D on the Laplacians and 3.22 on rand-N45 (zero guess), whose interval (10, 20) ends on eigenvalues: the seed is nearly
singular there and far nodes inherit its rounding.  No case is left out of the truncated comparison: the long-double
per-node reference breaks down on none.  Step counts of inexact solves are compared on the two Laplacians; rand-N45 would
iterate past its 45 unknowns.
"""
import numpy as np
import pytest

import krylov_reference as kr
import shifted_cases as sc
import shifted_krylov_reference as skr

KS = (1, 2, 5, 16, 33)


def _family(P, Z, q, ritz_c, rtol, maxit, dots=None):
    src, F, x0 = skr.start_of(P, q, Z, ritz_c)
    cols, _, seed, passes = skr.solve_family(P, Z, src, F, rtol, 0.0, maxit, dots=dots)
    return cols, x0, seed, passes


@pytest.mark.parametrize("warm", [False, True], ids=["zero", "ritz"])
@pytest.mark.parametrize("name", list(sc.PROBLEMS))
def test_every_node_walks_its_own_cocg_iterates(name, warm):
    A, Z, W, _ = sc.problem(name)
    N = A.shape[0]
    Q = sc.fk.seeded_subspace(N, sc.HOST_M)
    ritz = sc.ritz_guess(name, sc.HOST_M) if warm else None
    PL, PD = kr.Pencil(A, None, np.clongdouble), kr.Pencil(A, None, np.complex128)
    worst_ld = worst_64 = worst_node = 0.0
    drift = {k: 0.0 for k in KS}              # D of the case at step k: the family is ONE recurrence, the seed's rounding reaches every node
    found = []
    for j in range(sc.HOST_M):
        q = Q[:, j].astype(np.clongdouble)
        rc = None if ritz is None else ritz[j]
        for k in KS:
            fam, x0, seed, passes = _family(PL, Z, q, rc, 1e-14, k)
            f64, x064, _, _ = _family(PD, Z, Q[:, j], rc, 1e-14, k)
            assert seed == int(np.argmin(np.abs(Z.imag))) and passes == k
            for e, z in enumerate(Z):
                ref = kr.solve_column(PL, z, q, "cocg5", 1e-14, 0.0, k, x0=x0[e])
                assert ref.status == 0, (name, e, j, k)              # the per-node reference itself must not break down
                D = 0.0
                for chunks, sd in kr.DRIFT_ORDERS:
                    d = kr.solve_column(PD, z, Q[:, j], "cocg5", 1e-14, 0.0, k, x0=x064[e], dots=kr.Dots(N, chunks, sd))
                    assert d.steps == ref.steps
                    D = max(D, kr.rel_dist(d.x, ref.x))
                drift[k] = max(drift[k], D)
                assert fam[e].steps == ref.steps == k and fam[e].active and ref.active, (name, e, j, k)
                dist = kr.rel_dist(x0[e] + fam[e].dx, ref.x)
                found.append((e, j, k, dist))
                worst_ld = max(worst_ld, dist)
                worst_node = max(worst_node, dist / kr.tolerance(D))
                worst_64 = max(worst_64, kr.rel_dist(x064[e] + f64[e].dx, ref.x))
    print("shifted-host %s %s: D <= %.2e, long double shifted <= %.2e, complex128 shifted <= %.2e, worst share of a node's OWN "
          "32 D: %.2f" % (name, "ritz" if warm else "zero", max(drift.values()), worst_ld, worst_64, worst_node))
    for e, j, k, dist in found:
        assert dist <= kr.tolerance(drift[k]), (name, warm, e, j, k, dist, drift[k])


@pytest.mark.parametrize("warm", [False, True], ids=["zero", "ritz"])
@pytest.mark.parametrize("rtol,maxit", sc.INEXACT)
@pytest.mark.parametrize("name", ["lap-N336", "lap-N1080"])       # (rand-N45 would run past its 45 unknowns: truncated test only)
def test_inexact_step_counts_and_frozen_iterates(name, rtol, maxit, warm):
    """Every (node, column) stops at the step its own COCG stops at (and is frozen from then on); nodes that hit the cap
    report 5 in both.  (Iterates are compared in the truncated test: after 50 and more steps next to the spectrum the
    long-double forms themselves are 1e-5 apart, COCG's loss of conjugacy, and no longer tell a defect from rounding.)"""
    A, Z, W, _ = sc.problem(name)
    N = A.shape[0]
    Q = sc.fk.seeded_subspace(N, sc.HOST_M)
    ritz = sc.ritz_guess(name, sc.HOST_M) if warm else None
    PL, PD = kr.Pencil(A, None, np.clongdouble), kr.Pencil(A, None, np.complex128)
    steps = set()
    for j in range(sc.HOST_M):
        q = Q[:, j].astype(np.clongdouble)
        rc = None if ritz is None else ritz[j]
        fam, x0, seed, passes = _family(PL, Z, q, rc, rtol, maxit)
        for e, z in enumerate(Z):
            ref = kr.solve_column(PL, z, q, "cocg5", rtol, 0.0, maxit, x0=x0[e])
            assert ref.status == 0
            if min(ref.margin, fam[e].margin) < sc.MARGIN_MIN:
                continue
            assert (fam[e].steps, fam[e].active, fam[e].status) == (ref.steps, ref.active, ref.status), (name, e, j)
            assert kr.node_status([fam[e]], rtol, 0.0) == kr.node_status([ref], rtol, 0.0)
            steps.add(ref.steps)
        # one product per step of the slowest node, plus the one in which its stop is seen unless the cap came first
        mx = max(f.steps for f in fam)
        assert mx <= passes <= min(mx + 1, maxit)
    assert len(steps) >= 3, steps                 # the nodes do freeze at different steps


def test_edge_rules():
    A, Z, W, _ = sc.problem("rand-N45")
    P = kr.Pencil(A, None, np.clongdouble)
    q = np.random.default_rng(3).standard_normal(45)
    one = [1.0] * len(Z)
    zero, acc, _, passes = skr.solve_family(P, Z, np.zeros(45), one, 1e-3, 0.0, 50)
    assert all(c.steps == 0 and c.status == 0 and not c.active for c in zero) and not acc.any() and passes == 1
    masked, acc, _, _ = skr.solve_family(P, Z, q, one, 1e-3, 0.0, 50, masked=True)
    assert all(c.steps == 0 and not c.active for c in masked) and not acc.any()
    bad = q.copy(); bad[3] = np.nan
    nan, _, _, _ = skr.solve_family(P, Z, bad, one, 1e-3, 0.0, 50)
    assert all(c.status == kr.BREAKDOWN and c.steps == 0 and not c.active for c in nan)
    assert kr.node_status(nan, 1e-3, 0.0) == kr.NO_CONVERGENCE
    capped, _, _, passes = skr.solve_family(P, Z, q, one, 1e-14, 0.0, 4)
    assert all(c.steps == 4 and c.active for c in capped) and passes == 4
    # seed breakdown p^T S p = 0: S = -A = diag(-1 - i, 1 + i) is outside the real-A family but exercises the rule
    A2 = np.diag([1.0 + 1.0j, -1.0 - 1.0j])
    brk, _, _, _ = skr.solve_family(kr.Pencil(A2, None, np.clongdouble), [0.0, 0.5j], np.array([1.0, 1.0]), [1.0, 1.0], 1e-3, 0.0, 50)
    assert all(c.status == kr.BREAKDOWN and not c.active and c.steps == 0 for c in brk)


def test_sweep_cases_are_decidable():
    for family in sc.FAMILIES:
        for rtol, maxit in sc.INEXACT[:1]:
            c = sc.sweep_case("lap-N336", family, rtol, maxit, 9, True)
            assert c.decided.all() and c.fp64_steps_agree
            print("shifted-sweep-case lap-N336 family=%s rtol=%g drift %.2e" % (family, rtol, max(c.drift.values())))
