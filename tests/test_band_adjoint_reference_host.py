"""The order of operations of the adjoint band substitution, pinned on the CPU before any GPU run: the numpy restatement of
the blocked band LU with block-deferred interchanges (tests/band_adjoint_reference.py) against numpy.linalg.solve on random
unsymmetric complex band matrices with a zero diagonal (every column exchanges rows, many of them across a block boundary).

Bars: the forward solve 1e-12 relative; the adjoint solve 1e-12 x cond_1(S) (partial pivoting is backward stable for S, and
the adjoint substitution inherits the factors' backward error, so its forward error scales with the condition number)."""
import numpy as np
import pytest

import band_adjoint_reference as bar

# (N, kl, ku, block, seed, zero_every): N = 37 ragged last block; N = 40 a multiple of the block; kl > block: the left-looking update
# spans several blocks; kl = ku = 1 with a last block of one row
CASES = [(37, 5, 3, 8, 1, 1), (40, 5, 3, 8, 2, 1), (37, 5, 3, 4, 3, 1), (41, 9, 2, 4, 4, 1), (33, 1, 1, 8, 5, 2), (30, 3, 7, 8, 6, 1)]

_cache = {}


def _case(params):
    if params not in _cache:
        N, kl, ku, nb, seed, zero_every = params
        S = bar.random_band(N, kl, ku, seed, zero_every)
        LU, piv = bar.band_lu_blocked(S, kl, ku, nb)
        rng = np.random.default_rng(100 + seed)
        X = rng.standard_normal((N, 5)) + 1j * rng.standard_normal((N, 5))
        _cache[params] = (S, LU, piv, X, float(np.real(np.linalg.cond(S, 1))))
    return _cache[params]


@pytest.mark.parametrize("params", CASES)
def test_pivoting_is_genuine(params):
    N, kl, ku, nb = params[:4]
    _, _, piv, _, _ = _case(params)
    assert (piv != np.arange(N)).sum() >= N // 4
    assert (piv <= np.minimum(N - 1, (np.arange(N) // nb + 1) * nb + kl - 1)).all()          # inside [K0, nr)
    if nb < N and kl > 1:
        assert (piv >= (np.arange(N) // nb + 1) * nb).any()                                    # some cross their block's end


@pytest.mark.parametrize("params", CASES)
def test_forward_solve(params):
    N, kl, ku, nb = params[:4]
    S, LU, piv, X, cond = _case(params)
    want = np.linalg.solve(S, X)
    got = bar.solve_forward(LU, piv, kl, ku, nb, X)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("forward err %.2e cond %.1e" % (err, cond))
    assert err <= 1e-12


@pytest.mark.parametrize("params", CASES)
def test_adjoint_solve(params):
    N, kl, ku, nb = params[:4]
    S, LU, piv, X, cond = _case(params)
    want = np.linalg.solve(S.conj().T, X)
    got = bar.solve_adjoint(LU, piv, kl, ku, nb, X)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("adjoint err %.2e cond %.1e" % (err, cond))
    assert err <= 1e-12 * cond


def test_forward_order_of_the_interchanges_is_not_the_inverse():
    """the reversed order is what the test above checks: composing a block's interchanges first to last gives another answer"""
    params = CASES[0]
    N, kl, ku, nb = params[:4]
    S, LU, piv, X, _ = _case(params)
    want = np.linalg.solve(S.conj().T, X)
    wrong = bar.solve_adjoint(LU, piv, kl, ku, nb, X, reverse_swaps=False)
    assert np.linalg.norm(wrong - want) / np.linalg.norm(want) > 1e-3


def test_factors_reproduce_the_matrix():
    """S = P_0 L_0 P_1 L_1 ... U, block by block"""
    params = CASES[0]
    N, kl, ku, nb = params[:4]
    S, LU, piv, _, _ = _case(params)
    M = np.triu(LU)
    for K0 in reversed(range(0, N, nb)):
        Kend = min(N, K0 + nb)
        Lb = np.eye(N, dtype=complex)
        Lb[K0:, K0:Kend] += np.tril(LU[K0:, K0:Kend], -1)
        M = Lb @ M
        for j in range(Kend - 1, K0 - 1, -1):
            if piv[j] != j:
                M[[j, piv[j]]] = M[[piv[j], j]]
    assert np.abs(M - S).max() <= 1e-12 * np.abs(S).max()
