"""GPU: the dual variant of Benson's algorithm with the canonical optimal points handed to the LP engine PER CALL
(BSLV_VLP_CANONICAL_CALL of bslv_vlp_solve_dual2, vlp.solve_primal(.., canonical="call")): the way to them on an LP engine in the
revised form (BSLV_LP_REV=1), whose tie phase is k_select_tie_obj_rev.

Known answers: the decoy problems of canonical_obj_cases.py have an upper image with exactly the q vertices v_k = 2 (1 - e_k).  In the
tableau form the per-call flag must give what the engine-wide flag gives.  On covering_vlp(40, 20, 4, 9) in the revised form the points
of the upper image without a partner among the primal variant's vertices at poly_harness.DEFAULT_TOL must not be more with the flag on
than with it off -- tests/test_dual_variant_canonical_gpu.py's condition for the tableau form."""
import json

import numpy as np
import pytest

import canonical_obj_cases as co
import poly_harness as ph
from bensolve_amd import synth, vlp
from test_dual_variant_canonical_gpu import EPS, ZERO, _digest, _points, _solve, _unpartnered

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", [1, 64])
@pytest.mark.parametrize("q", [3, 4])
def test_revised_form_decoy_points_are_the_vertices(monkeypatch, q, batch):
    monkeypatch.setenv("BSLV_LP_REV", "1")
    prob = co.decoy_vlp(q)
    V = co.decoy_vertices(q)
    off = _solve(prob, False, batch)
    on = _solve(prob, "call", batch)
    X = _points(on)
    print("decoy-%d batch %d, revised form: %d points of the upper image with the flag off, %d with it on; LPs %d / %d; tie phase %s"
          % (q, batch, len(_points(off)), len(X), off["lps"], on["lps"], on["canonical_obj"]))
    assert off["canonical_obj"] == ZERO
    assert on["canonical_obj"]["capped"] == 0 and on["canonical_obj"]["entered"] > 0
    assert len(X) == q, X
    for v in V:
        assert np.abs(X - v).max(axis=1).min() <= 1e-9, (v, X)


@pytest.mark.parametrize("name", ["decoy-3", "covering-40x20x4"])
def test_tableau_form_the_call_is_the_switch(name):
    prob = co.decoy_vlp(3) if name == "decoy-3" else synth.covering_vlp(40, 20, 4, 9)
    flag, call = _solve(prob, True), _solve(prob, "call")
    print("%s, tableau form: LPs %d / %d; tie phase %s / %s" % (name, flag["lps"], call["lps"], flag["canonical_obj"], call["canonical_obj"]))
    assert _digest(ph.canonical(call["dump"], decimals=6)) == _digest(ph.canonical(flag["dump"], decimals=6))
    assert call["lps"] == flag["lps"] and call["canonical_obj"] == flag["canonical_obj"]
    assert call["canonical_obj"]["entered"] > 0


def test_revised_form_covering_run_off_and_on_against_the_primal_variant(monkeypatch):
    prob = synth.covering_vlp(40, 20, 4, 9)
    ref = _points(_solve(prob, alg="primal"))
    monkeypatch.setenv("BSLV_LP_REV", "1")
    off, on = _solve(prob, False), _solve(prob, "call")
    n_off, n_on = _unpartnered(_points(off), ref, ph.DEFAULT_TOL), _unpartnered(_points(on), ref, ph.DEFAULT_TOL)
    cs = on["canonical_obj"]
    print(json.dumps(dict(problem="covering_vlp(40, 20, 4, 9)", form="revised", batch=64, eps=EPS, tol=ph.DEFAULT_TOL, primal_variant_vertices=len(ref),
                          off=dict(unpartnered=n_off, points=len(_points(off)), lps=int(off["lps"]), steps=int(off["steps"])),
                          on=dict(unpartnered=n_on, points=len(_points(on)), lps=int(on["lps"]), steps=int(on["steps"]), tie=cs))))
    assert off["canonical_obj"] == ZERO
    assert cs["entered"] > 0 and cs["capped"] == 0
    assert n_on <= n_off, "points without a partner at %g: %d with the flag on, %d with it off" % (ph.DEFAULT_TOL, n_on, n_off)


@pytest.mark.parametrize("form", ["revised", "tableau"])
def test_environment_switch(monkeypatch, form):
    if form == "revised":
        monkeypatch.setenv("BSLV_LP_REV", "1")
    prob = co.decoy_vlp(3)
    flag = _solve(prob, "call")
    monkeypatch.setenv("BSLV_CANONICAL_OBJ_CALL", "1")
    env = _solve(prob, False)
    assert _digest(ph.canonical(env["dump"], decimals=6)) == _digest(ph.canonical(flag["dump"], decimals=6))
    assert env["canonical_obj"] == flag["canonical_obj"] and env["lps"] == flag["lps"]
    assert env["canonical_obj"]["entered"] > 0
