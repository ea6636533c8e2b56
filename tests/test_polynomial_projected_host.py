"""feast_polynomial(..., method="projected"), the host half: what the numpy restatement of the driver (polynomial_projected_reference)
does on the dense driver cases and on the two damped sparse cases -- the expectation the device test is held to --, the rule
under which a loop count may be pinned, a case on which the naive selection stagnates while the specified one converges, and
the keyword validation, which touches no device."""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import polynomial_cases as pc
import polynomial_projected_reference as ppr
import polynomial_reference as pr
import polynomial_sparse_cases as sc


def _clears(history, fpm3):
    """the history clears 10^-fpm3 by a factor >= 10 on both sides at the last step"""
    tol = 10.0 ** -fpm3
    return history[-1] <= tol / 10 and all(e >= 10 * tol for e in history[:-1])


@pytest.mark.parametrize("seed", ppr.SEEDS)
@pytest.mark.parametrize("params", pc.DRIVER_CASES, ids=pc.DRIVER_IDS)
def test_restatement_on_the_driver_cases(params, seed):
    N, d, k, _, monic = params
    key = (N, d, k, monic)
    fpm3, loop = ppr.DENSE_PINS[key]
    case = pc.make_case(*key)
    out = ppr.dense_run(key, k + 2, seed, fpm3)
    err = pr.match_error(out["lam"], case["lam_in"])
    print("loop %d history %s rank %s set aside %s eigenvalue error %.2e" % (out["loop"], ["%.1e" % e for e in out["eps_history"]],
                                                                            out["rank"], out["set_aside"], err))
    assert out["info"] == 0 and out["M"] == k
    assert err <= 1e-8
    assert out["loop"] == loop
    assert _clears(out["eps_history"], fpm3)
    assert out["candidates"] == [d * r for r in out["rank"]] and max(out["rank"]) <= k + 2
    # the backward error the run reports is the one numpy computes on its vectors
    assert np.allclose(out["res"], pr.backward_error(case["coeffs"], out["lam"], out["q"]), rtol=1e-3, atol=1e-16)
    # ... and the count does not hang on rounding
    pert = ppr.dense_run(key, k + 2, seed, fpm3, False, 1e-14)
    assert pert["loop"] == loop and _clears(pert["eps_history"], fpm3)


@pytest.mark.parametrize("monic", [True, False])
def test_naive_selection_stagnates(monic):
    """The reduced polynomial has d r Ritz values for r columns; the surplus ones land inside the circle.  "The m nearest the
    centre, nothing set aside" keeps them and stays at 1e-2 for 20 loops; the specified selection stops at loop 2."""
    key = (70, 2, 6, monic)
    naive = ppr.dense_run(key, 8, 1, pc.FPM3, True)
    good = ppr.dense_run(key, 8, 1, pc.FPM3, False)
    print("naive: info %d loop %d last %s; specified: loop %d %s" % (naive["info"], naive["loop"], ["%.1e" % e for e in naive["eps_history"][-3:]],
                                                                   good["loop"], ["%.1e" % e for e in good["eps_history"]]))
    assert naive["info"] != 0 and naive["loop"] == 20 and min(naive["eps_history"]) > 1e-3
    assert good["info"] == 0 and good["loop"] == 2 and good["M"] == 6
    assert max(good["set_aside"]) >= 1          # the rule was needed, not idle


@pytest.mark.parametrize("name,scaled", sc.DRIVER_CASES, ids=sc.DRIVER_IDS)
def test_restatement_on_the_damped_cases(name, scaled):
    columns, seed, loop = ppr.DAMPED_PINS[(name, scaled)]
    case = sc.damped_case(name, scaled)
    out = ppr.damped_run(name, scaled, columns, seed)
    err = pr.match_error(out["lam"], case["lam_in"])
    print("loop %d history %s eigenvalue error %.2e" % (out["loop"], ["%.1e" % e for e in out["eps_history"]], err))
    assert out["info"] == 0 and out["M"] == case["k"] and err <= 1e-8
    assert out["loop"] == loop and _clears(out["eps_history"], sc.FPM3)
    pert = ppr.damped_run(name, scaled, columns, seed, sc.FPM3, 1e-14)
    assert pert["loop"] == loop and _clears(pert["eps_history"], sc.FPM3)


def test_selection_rules():
    """poly_select of the package against the restatement's, on a hand-made candidate list"""
    theta = np.array([0.1, 0.2 + 0.1j, 5.0, np.inf, -0.3j, 2.0, 0.05])
    be = np.array([1e-9, 5e-2, 1e-12, np.inf, 2e-3, 1e-3, 0.9])
    for keep in (3, 5, 7):
        sel, good, aside = fk.hip_backend.poly_select(theta, be, 0.0, 1.0, keep)
        rsel, rgood, raside = ppr.select(theta, be, 0.0, 1.0, keep)
        assert list(sel) == list(rsel) and list(good) == list(rgood) and aside == raside
    sel, good, aside = fk.hip_backend.poly_select(theta, be, 0.0, 1.0, 6)
    assert list(sel) == [0, 4, 1, 6, 5, 2]            # inside by backward error, then outside by distance; never the infinite one
    assert list(good) == [True, False, False, False, False, False] and aside == 3
    assert fk.api.POLY_SET_ASIDE == (1e-3, 100.0) and fk.hip_backend.POLY_SET_ASIDE is fk.api.POLY_SET_ASIDE


def _dense():
    return pc.make_case(70, 2, 6, True)["coeffs"]


@pytest.mark.parametrize("kw,word", [
    ({"method": "projection"}, "method"),
    ({"method": None}, "method"),
    ({"method": "projected", "residual": "reference"}, "residual"),
    ({"method": "projected", "ortho": "householder"}, "ortho"),
    ({"method": "linearised", "ortho": "householder"}, "ortho"),
    ({"method": "projected", "Q0": np.zeros((140, 16))}, "Q0"),
    ({"method": "projected", "Q0": np.zeros((70, 7))}, "Q0"),
])
def test_method_keyword_validation_is_host_only(kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    with pytest.raises(ValueError, match=word):
        fk.feast_polynomial(_dense(), pc.CENTER, pc.RADIUS, M0=8, **kw)
    assert fk.feast_pep is fk.feast_polynomial


def test_valid_keywords_reach_the_engine(monkeypatch):
    class Reached(Exception):
        pass

    def no_engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(fk.api, "_engine", no_engine)
    I = sp.identity(12, format="csr")
    for kw in ({"method": "projected"}, {"method": "projected", "ortho": "cholqr_rr", "Q0": np.ones((12, 3))},
               {"method": "projected", "solver": "sparse_direct"}, {"method": "linearised", "residual": "reference"}):
        with pytest.raises(Reached):
            fk.feast_polynomial([I, I, I], 0.0, 1.0, M0=3, **kw)
