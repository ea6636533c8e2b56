"""The block COCG restatement (block_cocg_reference.py) on the host: every case of block_cocg_cases.py against a sparse LU of
z B - A, its recurrence residual against the true one, its step counts against the per-column COCG restatement, and its own
complex128 drift D, which must leave the device comparison of test_gpu_block_cocg.py its meaning (tolerance(D) < 1e-6)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import krylov_reference as kr
import block_cocg_reference as br
import block_cocg_cases as bc


def _true_parts(c, e):
    """(right-hand side of node e, exact solution update, shifted matrix) in complex128"""
    N = c.A.shape[0]
    Bm = sp.identity(N, format="csr") if c.B is None else c.B
    z = c.Z[e]
    S = (z * Bm - c.A).tocsc()
    if c.ritz is None:
        R0 = Bm @ c.Q
    else:
        R0 = (c.A @ c.Q - (Bm @ c.Q) * c.ritz[None, :]) / (z - c.ritz)[None, :]
    if c.mask is not None:
        R0 = R0 * np.asarray(c.mask)[None, :]
    return R0, spl.splu(S).solve(R0.astype(np.complex128)), S


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_restatement_solves_the_shifted_systems(cid):
    c = bc.case(cid)
    for e, nd in enumerate(c.ref.nodes):
        R0, Xex, S = _true_parts(c, e)
        X = nd.X.astype(np.complex128)
        true_res = R0 - S @ X
        if nd.fallback is None:
            # the recurrence residual Q C is the true residual
            scale = np.linalg.norm(R0, axis=0).max()
            assert np.linalg.norm(true_res - nd.Rrec.astype(np.complex128)) <= 1e-8 * scale, (cid, e)
        rel = np.linalg.norm(true_res, axis=0) / np.maximum(np.linalg.norm(R0, axis=0), 1e-300)
        if nd.stop == br.CONVERGED or nd.fallback is not None:
            live = nd.r0norm > 0
            assert (rel[live] <= 1.01 * c.rtol + 1e-13).all(), (cid, e, rel)
            # ... so the iterate matches the direct solve to the stop tolerance (times the conditioning of S)
            cond = 1.0 / abs(c.Z[e].imag)
            err = np.linalg.norm(X - Xex, axis=0) / np.maximum(np.linalg.norm(Xex, axis=0), 1e-300)
            assert (err[live] <= 4.0 * cond * max(c.rtol, 1e-13)).all(), (cid, e, err.max())
    if cid.endswith("breakdown"):
        assert list(c.ref.steps) == [0] and list(c.ref.stop) == [br.BREAKDOWN] and not c.ref.status.any()


@pytest.mark.parametrize("cid", bc.CONVERGED)
def test_block_takes_no_more_steps_than_per_column_cocg(cid):
    c = bc.case(cid)
    P = kr.Pencil(c.A, c.B, np.complex128)
    for e, nd in enumerate(c.ref.nodes):
        R0 = _true_parts(c, e)[0]
        worst = max(kr.solve_column(P, c.Z[e], R0[:, j], "cocg_fused", c.rtol, 0.0, 4000).steps for j in range(c.m))
        print("block-steps %s node %d: block %d, per-column cocg %d" % (cid, e, nd.steps, worst))
        assert nd.stop == br.CONVERGED and nd.steps <= worst, (cid, e, nd.steps, worst)


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_drift_leaves_the_device_comparison_its_meaning(cid):
    c = bc.case(cid)
    print("block-drift %s D=%.3e" % (cid, c.drift))
    assert c.fp64_agree
    assert br.tolerance(c.drift) < 1e-6, (cid, c.drift)
