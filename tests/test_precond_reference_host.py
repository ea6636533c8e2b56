"""What the device comparison of test_gpu_precond.py rests on, asserted on the reference alone (no GPU): precond_reference.py
over the cases of precond_cases.py.

Measured here (long double against complex128 over krylov_reference.DRIFT_ORDERS with four splu column orders): every case
of precond_cases.CASES ends with status 0 and no active column; D <= 4.9e-14 (the warm start; <= 2.7e-14 on N = 1080,
<= 1.2e-14 on the tridiagonal case, <= 3.1e-15 elsewhere); the smallest stop margin 1.2e-3, no pair undecided; lock-steps 17,
27, 50, 51, 27, 37, 16, 16, 17, 21 in the order of the table.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import krylov_reference as kr
import precond_cases as pc
import precond_reference as pr
from test_gpu_primitives import sparse_pair

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_meets_the_conditions_of_the_device_comparison(name):
    c = pc.case(name)
    r = c.ref
    print("precond-host %s lock_steps=%d products=%d sweeps=%d rowmax=%s D=%s min margin=%.2e" %
          (name, r.lock_steps, r.products, r.sweeps, list(r.steps.max(axis=1)), c.drift, r.margin.min()))
    assert not any(col.active for row in r.cols for col in row) and not r.status.any()
    assert r.lock_steps < pc.MAXIT
    assert c.fp64_steps_agree
    for real in (True, False):
        assert 32.0 * c.drift[real] <= pc.POWER, (name, c.drift)
    for k in c.ks:
        assert 32.0 * c.trunc_drift[k] <= pc.POWER, (name, k, c.trunc_drift)
        assert (c.trunc[k][3] < pc.MARGIN_MIN).mean() <= pc.LEFT_OUT_MAX
    assert (~c.decided).mean() <= pc.LEFT_OUT_MAX
    # a node whose shift is its pivot has c_e = 0: the operator is the identity and it leaves after one step
    for e, p in enumerate(c.node_pivot):
        if complex(c.Z[e]) == c.pivots[p]:
            assert (r.steps[e] == 1).all()


@pytest.mark.parametrize("name", ["cfg3-N336-m16-r10", "ragged-nonsym-N323-m17-r8", "csr-I-N45-m7-r30"])
def test_identity_form_is_the_preconditioned_operator(name):
    """S^ v = v + (z_e - z_p) B M^-1 v equals S_e (M^-1 v) formed from the plain pencil, in long double, to 64 eps (fp64)."""
    c = pc.case(name)
    P = c.ref.pencil
    rng = np.random.default_rng(5)
    for e in (0, len(c.Z) - 1, 3):
        v = (rng.standard_normal(c.N) + 1j * rng.standard_normal(c.N)).astype(np.clongdouble)
        lhs = P.apply(c.Z[e], v)
        rhs = P.plain(c.Z[e], P.minv(c.node_pivot[e], v))
        assert kr.rel_dist(lhs, rhs) <= 64.0 * EPS, (name, e)
        assert kr.rel_dist(P.mul_pivot(c.node_pivot[e], P.minv(c.node_pivot[e], v)), v) <= 64.0 * EPS


@pytest.mark.parametrize("name", list(pc.CASES))
def test_true_residual_of_x_meets_its_target(name):
    """The fp64 residual b - S_e x of x = M^-1 u, recomputed on the host, is at most twice the column's target (the host
    recomputation rounds at about 1e-13 relative against rtol = 1e-10)."""
    c = pc.case(name)
    A = sp.csr_matrix(c.A).astype(np.complex128)
    B = sp.identity(c.N, format="csr", dtype=np.complex128) if c.B is None else sp.csr_matrix(c.B).astype(np.complex128)
    for e, z in enumerate(c.Z):
        for col, x in zip(c.ref.cols[e], c.ref.xs[e]):
            r = col.b.astype(np.complex128) - (complex(z) * (B @ x.astype(np.complex128)) - A @ x.astype(np.complex128))
            assert np.linalg.norm(r) <= 2.0 * float(col.target), (name, e)


def test_one_pivot_stalls_on_a_dense_spectrum():
    """The counter-example of DESIGN.md section 6v: on sparse_pair(333) the spectrum is dense inside (20, 30); under ONE pivot
    the two nodes nearest the axis do not converge within the cap at restart 8, and not at restart 30 either (120 steps); the
    pinned case converges because it takes two pivots.  complex128 (a stall is no matter of rounding)."""
    A, B = sparse_pair(333, 7)
    Z, W = pc.contour8(20.0, 30.0)
    Q = pc.fk.seeded_subspace(333, 2)
    piv, node_pivot = pc.pivots_of("arcs:1", Z)
    for restart, cap in ((8, 60), (30, 120)):
        r = pr.sweep(A, B, Q, Z, W, 2.0, piv, node_pivot, pc.RTOL, 0.0, cap, restart, dtype=np.complex128)
        stalled = [e for e, row in enumerate(r.cols) if any(col.active for col in row)]
        print("one pivot, restart %d: lock-steps %d, stalled nodes %s" % (restart, r.lock_steps, stalled))
        assert r.lock_steps == cap and stalled and set(stalled) <= {0, 1, 6, 7}, (restart, stalled)
    two = pc.case("csr-B-N333-m5-r30").ref
    assert two.lock_steps < 120 and not two.status.any()


def test_pivot_rules():
    assert pr.arc_pivots(8, 2) == ([0, 0, 0, 0, 1, 1, 1, 1], [1, 6])
    assert pr.arc_pivots(8, 1) == ([0] * 8, [3])
    assert pr.arc_pivots(16, 4)[1] == [1, 5, 10, 14]
    assert pr.arc_pivots(3, 5) == ([0, 1, 2], [0, 1, 2])
    for ne in range(1, 20):
        for k in range(1, ne + 3):
            node_pivot, pivot_node = pr.arc_pivots(ne, k)
            kk = min(k, ne)
            assert sorted(set(node_pivot)) == list(range(kk)) and node_pivot == sorted(node_pivot)
            counts = [node_pivot.count(a) for a in range(kk)]
            assert max(counts) - min(counts) <= 1
            assert all(node_pivot[pivot_node[a]] == a for a in range(kk))
            if kk == 2 and ne % 2 == 0:
                assert pivot_node[1] == ne - 1 - pivot_node[0]                      # two halves: the pivots mirror each other
    Z = np.array([1 + 1j, 2 + 2j, 3 + 1j])
    assert pr.nearest_pivots(Z, [3 + 0.5j, 1 + 0.5j]) == [1, 0, 0]
    # the driver's plan (hip_backend.precond_plan) states the same rules
    from feastkit_jl_amd.hip_backend import precond_plan
    Z8, _ = pc.contour8(0.0, 0.5)
    assert precond_plan(Z8, 2) == ([complex(Z8[1]), complex(Z8[6])], [0, 0, 0, 0, 1, 1, 1, 1])
    assert precond_plan(Z8, [0.25 + 0.25j, 0.4 + 0.1j])[1] == pr.nearest_pivots(Z8, [0.25 + 0.25j, 0.4 + 0.1j])
