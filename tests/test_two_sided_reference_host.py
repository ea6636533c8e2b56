"""Two-sided FEAST on the host: the restatement of the loop (tests/two_sided_reference.py) converges on every prescribed-
spectrum case, and the keyword validation of feast_general(two_sided=True) needs no GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import feastkit_jl_amd as fk
import two_sided_cases as tc
from two_sided_reference import reference_run, residuals


@pytest.mark.parametrize("params", tc.PARAMS, ids=tc.IDS)
def test_restatement_converges(params):
    case = tc.make_case(*params)
    ref = reference_run(params)
    print("loops %d epsout %.2e cond(X) %.1f" % (ref["loop"], ref.get("epsout", np.inf), case["cond_X"]))
    assert ref["info"] == 0 and ref["loop"] <= 20 and ref["epsout"] <= 1e-12
    assert ref["M"] == case["n_in"]
    assert np.abs(ref["lam"] - case["lam_in"]).max() <= 1e-10
    Y = ref["Y"] / np.linalg.norm(ref["Y"], axis=0)
    rr, rl = residuals(case["A"].astype(complex), case["B"], ref["lam"], ref["X"], Y)
    print("res_R %.2e res_L %.2e" % (rr.max(), rl.max()))
    assert rr.max() <= 1e-10 and rl.max() <= 1e-10


@pytest.mark.parametrize("kw,word", [(dict(solver="krylov"), "solver"), (dict(inner_precision=32), "inner_precision"),
                                     (dict(group=object()), "group"), (dict(direct_nodes=[0]), "direct_nodes")])
def test_keyword_validation_is_host_only(kw, word, monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    A = np.diag(np.arange(1.0, 9.0))
    with pytest.raises(ValueError, match=word):
        fk.feast_general(A, None, 0.0, 1.0, M0=4, two_sided=True, **kw)


def test_sparse_input_is_refused(monkeypatch):
    monkeypatch.setattr(fk.api, "_engine", lambda *a, **k: pytest.fail("an engine was created before the validation"))
    with pytest.raises(ValueError, match="dense"):
        fk.feast_general(sp.identity(8, format="csr"), None, 0.0, 1.0, M0=4, two_sided=True)


def test_result_field_defaults():
    r = fk.FeastResult(np.zeros(0), np.zeros((3, 0)), 0, np.zeros(0), 0, 0.0, 0, {})
    assert r.q_left is None
