"""GPU: the Benson driver with cuts from canonical duals on a REVISED LP engine (BSLV_LP_REV=1 with bslv_benson_set_canonical(1)): the
driver hands the direction to every batch of P2 LPs and to its retries by bslv_lpq_solve_batch_canonical, the engine has no switch there.

Known answer: the octahedron VLP -- every cut has to be one of its seven facets, by tests/test_benson_canonical_gpu.py's own check.
covering_vlp(40, 20, 4, 9) to termination has to end in the sets of the tableau-form canonical run at poly_harness.DEFAULT_TOL.  Both
again with BSLV_FORCE_RETRY=1, where every other LP goes through the retry stages."""
import ctypes

import numpy as np
import pytest

import poly_harness as ph
import test_benson_canonical_gpu as tb
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine

pytestmark = pytest.mark.gpu
BATCH = 64


def _is_revised(eng):
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    return int(eng.lib.bslv_lpq_is_revised(eng._lp_h))


@pytest.fixture
def revised(monkeypatch):
    """every BensonEngine of the test gets a revised LP engine -- asserted on an engine of its own"""
    monkeypatch.setenv("BSLV_LP_REV", "1")
    eng = BensonEngine(tb._known("octahedron")[0], eps=tb.EPS, pool_slots=16)
    try:
        assert _is_revised(eng) == 1
        eng.set_canonical(1)                   # (no BSLV_E_ARG any more)
        assert eng.get_canonical() == 1
    finally:
        eng.close()


@pytest.mark.parametrize("retry", [False, True])
@pytest.mark.parametrize("policy", [1, 3])
def test_every_cut_of_the_octahedron_is_a_facet(revised, monkeypatch, policy, retry):
    if retry:
        monkeypatch.setenv("BSLV_FORCE_RETRY", "1")
    tb.test_every_cut_is_a_facet("octahedron", policy, BATCH)
    _, _, cs = tb._run_recording_cuts(tb._known("octahedron")[0], policy, BATCH, True)
    print("benson_rev_canonical octahedron policy %d retry %s: tie phase %s" % (policy, retry, cs["total"]))
    assert cs["total"]["tie_pivots"] > 0 and cs["total"]["capped"] == 0


def test_environment_switches_create_and_run(monkeypatch):
    """BSLV_CANONICAL_DUAL=1 with BSLV_LP_REV=1 no longer fails at create"""
    monkeypatch.setenv("BSLV_LP_REV", "1")
    monkeypatch.setenv("BSLV_CANONICAL_DUAL", "1")
    eng = BensonEngine(tb._known("octahedron")[0], eps=tb.EPS, pool_slots=4 * BATCH + 64)
    try:
        assert _is_revised(eng) == 1 and eng.get_canonical() == 1
        assert eng.start() == 0
        eng.run(BATCH)
        assert eng.canonical_stats()["total"]["tie_pivots"] > 0
    finally:
        eng.close()


_tableau = {}


def _tableau_run(prob, policy):
    if policy not in _tableau:
        _tableau[policy] = tb._to_termination(prob, policy, BATCH, 1)[0]
    return _tableau[policy]


@pytest.mark.parametrize("retry", [False, True])
def test_covering_run_ends_in_the_sets_of_the_tableau_form(monkeypatch, retry):
    prob = synth.covering_vlp(40, 20, 4, 9)
    policy = 1
    monkeypatch.delenv("BSLV_LP_REV", raising=False)
    exp = _tableau_run(prob, policy)
    monkeypatch.setenv("BSLV_LP_REV", "1")
    if retry:
        monkeypatch.setenv("BSLV_FORCE_RETRY", "1")
    eng = BensonEngine(prob, eps=tb.EPS, pool_slots=4 * BATCH + 64)
    assert _is_revised(eng) == 1
    eng.close()
    got, tot, cs = tb._to_termination(prob, policy, BATCH, 1)
    print("benson_rev_canonical covering_vlp(40, 20, 4, 9) retry %s: %s; tie phase %s; %d vertices, %d facets (tableau form: %d, %d)" % (
        retry, tot, cs, len(got["X"]), len(got["Y"]), len(exp["X"]), len(exp["Y"])))
    assert cs["tie_pivots"] > 0 and cs["capped"] == 0
    assert ph.assert_benson_results_agree(got, exp, tol=ph.DEFAULT_TOL) == "exact"
