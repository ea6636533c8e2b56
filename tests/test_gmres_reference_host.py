"""The batch-level GMRES restatement (gmres_reference.py) checked against the oracle's restarted GMRES and against a dense
least-squares minimiser over the explicit Krylov basis, and the conditions on the inputs of test_gpu_gmres_steps.py
(gmres_cases.py) that keep the device comparison from hiding a failure: discriminating power (32 D <= 1e-7, D the drift of
the restatement in complex128 against long double over four summation orders), decidable stops (at most 2 % of the (node,
column) pairs of a case within 1e-6 of a stop threshold; the reference leaves out none) and fp64 step counts that agree
with the long-double ones.  No GPU."""
import numpy as np
import pytest

import feast_oracle as fo
import gmres_cases as gc
import gmres_reference as gr
import krylov_reference as kr
from test_gpu_primitives import sparse_pair


def _dense_S(A, B, z):
    A = A.toarray()
    return z * (np.eye(A.shape[0]) if B is None else B.toarray()) - A


@pytest.mark.parametrize("cplx,bid", [(False, False), (False, True), (True, False)])
def test_restatement_is_the_minimiser_over_the_krylov_space(cplx, bid):
    """In long double, one cycle of k steps from a zero guess gives argmin |b - S x| over span(b, S b, ..., S^(k-1) b), and
    the restarted run cut at any step is the oracle's restarted GMRES (modified Gram-Schmidt, fp64) cut there."""
    N = 60
    A, B = sparse_pair(N, 3, cplx=cplx, b_identity=bid)
    z = -3.0 + 2.0j
    S = _dense_S(A, B, z)
    rng = np.random.default_rng(4)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    P = kr.Pencil(A, B, np.clongdouble)
    one = gr.solve_batch(P, [z], b[:, None], None, 1e-14, 0.0, 6, 30, keep_history=True)
    K = np.zeros((N, 6), complex)
    v = b.copy()
    for k in range(6):
        K[:, k] = v / np.linalg.norm(v)
        v = S @ K[:, k]
        coef = np.linalg.lstsq(S @ K[:, :k + 1], b, rcond=None)[0]
        assert kr.rel_dist(one.cols[0][0].history[k + 1][0], K[:, :k + 1] @ coef) <= 1e-11, k
    run = gr.solve_batch(P, [z], b[:, None], None, 1e-14, 0.0, 23, 5, keep_history=True)
    for k in (1, 4, 5, 6, 10, 11, 23):
        xo, ok, its = fo.gmres_restarted(lambda x: S @ x, b, 1e-14, 0.0, k, 5)
        x, steps, status, active, _ = gr.truncated(run, run.cols[0][0], k)
        assert its == steps == k and active and not ok and status == 0
        assert kr.rel_dist(x, xo) <= 1e-12, (k, kr.rel_dist(x, xo))
    assert [gr.truncated_products(run, k) for k in (1, 4, 5, 6, 10, 11)] == [3, 6, 7, 9, 13, 15]
    for dtype, tol in ((np.clongdouble, 1e-11), (np.complex128, 1e-10)):
        full = gr.solve_batch(kr.Pencil(A, B, dtype), [z], b[:, None], None, 1e-13, 0.0, 500, 20)
        col = full.cols[0][0]
        assert col.status == 0 and not col.active and 0 < col.steps < 500 and col.rnorm <= 1e-13 * col.r0norm
        assert gr.node_status(full.cols[0]) == 0 and full.products == full.lock_steps + full.cycles
        assert kr.rel_dist(col.x.astype(np.complex128), np.linalg.solve(S, b)) <= tol
        xo, ok, its = fo.gmres_restarted(lambda x: S @ x, b, 1e-13, 0.0, 500, 20)
        assert ok and its == col.steps


def test_edge_rules():
    A, B = sparse_pair(40, 6)
    P = kr.Pencil(A, B, np.clongdouble)
    z = -3.0 + 2.0j
    b = np.random.default_rng(1).standard_normal(40)
    bad = b.copy(); bad[3] = np.nan
    rhs = np.stack([b, np.zeros(40), bad, 1e-9 * b / np.linalg.norm(b)], axis=1)
    r = gr.solve_batch(P, [z], rhs, None, 3e-2, 1e-6, 50, 0)
    live, zero, nan, tiny = r.cols[0]
    assert live.status == 0 and not live.active and live.steps > 0
    assert zero.steps == 0 and zero.status == 0 and not zero.active and not zero.x.any()
    assert nan.steps == 0 and nan.status == kr.BREAKDOWN and not nan.active
    assert tiny.steps == 0 and tiny.status == 0 and not tiny.active and not tiny.x.any()
    assert gr.node_status([live, zero, tiny]) == 0 and gr.node_status([nan]) == kr.NO_CONVERGENCE
    # restart 0 and 1 are GMRES(2); the cap cuts the same sequence short and leaves the node at 5
    two = gr.solve_batch(P, [z], rhs[:, :1], None, 1e-14, 0.0, 9, 2, keep_history=True)
    for restart in (0, 1):
        other = gr.solve_batch(P, [z], rhs[:, :1], None, 1e-14, 0.0, 9, restart)
        assert np.array_equal(other.cols[0][0].x, two.cols[0][0].x) and other.products == two.products == 9 + 5 + 1
    cut = gr.solve_batch(P, [z], rhs[:, :1], None, 1e-14, 0.0, 3, 2)
    assert cut.lock_steps == 3 and cut.cols[0][0].active and gr.node_status(cut.cols[0]) == kr.NO_CONVERGENCE
    assert np.array_equal(gr.truncated(two, two.cols[0][0], 3)[0], cut.cols[0][0].x)
    # the warm start is q / (z - ritz); the mask changes nothing
    Q = rhs[:, :1].astype(complex)
    warm = gr.sweep(A, B, Q, [z], [1.0], 1.0, False, 1e-14, 0.0, 0, 8, ritz=np.array([2.5]), mask=[0], pencil=P)
    assert warm.steps[0, 0] == 0 and kr.rel_dist(warm.out[:, 0], Q[:, 0] / (z - 2.5)) <= 1e-15 and warm.products == 1


@pytest.mark.parametrize("near", [False, True], ids=["far", "near"])
@pytest.mark.parametrize("name", list(gc.TRUNC))
def test_truncated_inputs_have_discriminating_power(name, near):
    c = gc.trunc_case(name, near)
    for k in c.ks:
        assert 32.0 * c.drift[k] <= gc.POWER, (name, near, k, c.drift[k])
        assert all(w[4] >= gc.MARGIN_MIN for w in c.want[k])              # the reference leaves out no column
        assert all(w[1] == k and w[3] for w in c.want[k])                  # genuinely truncated: k steps, still above the target
        assert c.products[k] == k + -(-k // c.mr) + 1
    mr = c.mr
    assert any(k % mr for k in c.ks) and any(k % mr == 0 for k in c.ks) and any(k % mr == 1 and k > mr for k in c.ks)


@pytest.mark.parametrize("restart", gc.STOP_RESTARTS)
def test_stop_inputs_stop_at_different_steps_and_are_decidable(restart):
    for rtol, atol in gc.STOP_SETTINGS:
        c = gc.stop_case(rtol, atol, restart)
        steps = c.ref.steps[0]
        assert steps[5] == 0 and not c.ref.out[:, 5].any()                 # the zero column
        if atol > 0:
            assert steps[11] == 0 and c.ref.cols[0][11].r0norm <= atol     # below atol from the start
        assert len(set(steps)) >= 6, steps
        assert list(steps[:4]) == [1, 2, 4, 8][:4] or rtol > 1e-3          # a sum of 2^j eigenvectors is exhausted after 2^j steps
        assert list(c.ref.status) == [0] and c.decided.all() and c.fp64_steps_agree
        assert 32.0 * max(c.drift.values()) <= gc.POWER
        # columns leave inside a cycle while others go on: the lock-steps are the slowest column's, and the cycle that it
        # ends early is not run to its end
        assert c.ref.lock_steps == [steps.max()] and c.ref.products == steps.max() + -(-steps.max() // max(restart, 2)) + 1


def test_exhaustion_stops_on_the_estimate_at_the_step_that_exhausts_the_space():
    for name in gc.EXHAUST:
        c = gc.exhaust_case(name)
        assert (c.ref.steps == c.dim).all() and list(c.ref.status) == [0]
        assert c.decided.all() and c.fp64_steps_agree and (c.ref.margin > 0.5).all()
        assert 32.0 * max(c.drift.values()) <= gc.POWER
        S = _dense_S(c.A, c.B, c.Z[0])
        assert kr.block_dist(c.ref.out.astype(complex), np.linalg.solve(S, c.Q)) <= 1e-10


@pytest.mark.parametrize("case", range(1, 5))
def test_sweep_inputs_are_decidable_and_discriminating(case):
    kind, m, warm, setting = gc.SWEEPS[case]
    c = gc.sweep_case(kind, m, warm, setting)
    assert c.decided.all() and c.fp64_steps_agree and c.ref.reactivated == 0
    for real in (True, False):
        assert 32.0 * c.drift[real] <= gc.POWER, (case, real, c.drift[real])
    if setting[1] == 12:
        assert (c.ref.steps == 12).all() and list(c.ref.status) == [kr.NO_CONVERGENCE] * 8       # every node capped
    else:
        assert len(set(c.ref.steps.ravel())) >= 2 and list(c.ref.status) == [0] * 8


def test_batch_size_reaches_a_column_only_through_the_step_counter():
    """The capped sweep under node batches of 8, 3 and 1: every batch has its own counter (12 lock-steps each, so 15, 45 and
    120 products), and the iterates and steps are the same bits.  No column's steps differ between the batch sizes, and
    none can in a reference: an active column takes every lock-step of its batch, so a difference needs a column that left
    on the Givens estimate and is reactivated by the next true residual -- a rounding event (the two norms are equal in
    exact arithmetic) that long double does not reproduce and whose margin is below 1e-6 (gmres_reference.py)."""
    kind, m, warm, setting = gc.MASK_SWEEP
    runs = {b: gc.sweep_case(kind, m, warm, setting, b) for b in gc.BATCHES}
    assert [runs[b].ref.lock_steps for b in gc.BATCHES] == [[12], [12] * 3, [12] * 8]
    assert [runs[b].ref.products for b in gc.BATCHES] == [15, 45, 120]
    for b in (3, 1):
        assert np.array_equal(runs[b].ref.steps, runs[8].ref.steps) and np.array_equal(runs[b].ref.out, runs[8].ref.out)
        assert np.array_equal(runs[b].ref.status, runs[8].ref.status)
    # not capped: the batches end when their own slowest column does (30, the node next to the real axis, is in the last)
    free = {b: gc.sweep_case("hermitian", 24, True, gc.SWEEP_SETTINGS[2], b).ref for b in (8, 3)}
    assert free[8].lock_steps == [30] and free[3].lock_steps == [int(free[8].steps[e0:e0 + 3].max()) for e0 in (0, 3, 6)]
    assert free[8].products == 32 and free[3].products == sum(free[3].lock_steps) + 6
    assert np.array_equal(free[3].steps, free[8].steps) and np.array_equal(free[3].out, free[8].out)
    assert gc.budget_mb(1080, 24, 10, 3) == 19 and gc.budget_mb(500, 4, 20, 1) == 3
