"""GPU: the dual variant of Benson's algorithm with cuts from canonical optimal points (BSLV_VLP_CANONICAL of bslv_vlp_solve_dual2).
Everything goes through vlp.solve_primal(alg_phase2="dual", ...).

Known answers: the decoy problems of canonical_obj_cases.py have an upper image with exactly the q vertices v_k = 2 (1 - e_k), and
every other column of P is the image of a vertex of the feasible set that lies on a face of the image.  With the flag on the points of
the upper image in the result are exactly the v_k, for batches of 1 and 64.

Measured, not promised: covering_vlp(40, 20, 4, 9) to termination with the flag off and on against the primal variant's run -- the
upper-image points of the dual run without a partner among the primal run's vertices at poly_harness.DEFAULT_TOL must not be more
with the flag on than with it off; the counts are printed and, where BSLV_RECORD_DIR names a directory, written to canonical_obj.json
there (profiles/canonical_obj_parity.txt holds the run recorded with the feature)."""
import hashlib
import json
import os

import numpy as np
import pytest

import canonical_cases as cc
import canonical_obj_cases as co
import poly_harness as ph
from bensolve_amd import synth, vlp

pytestmark = pytest.mark.gpu
EPS = 1e-9
ZERO = dict(entered=0, tie_iters=0, unbounded=0, capped=0)


def _solve(prob, canonical=False, batch=64, alg="dual"):
    out = vlp.solve_primal(prob, eps_benson_phase2=EPS, batch=batch, alg_phase2=alg, canonical=canonical)
    assert out["status"] == "optimal", out
    return out


def _points(out):
    """the used non-ideal points of the upper image"""
    d = out["dump"]
    return d["X"][(d["pu"] != 0) & (d["pi"] == 0)]


def _digest(can, decimals=6):
    """SHA-256 over the whole canonical dump (tests/test_benson_canonical_gpu.py's)"""
    h = hashlib.sha256()
    for k in sorted(can):
        v = can[k]
        if isinstance(v, np.ndarray):
            a = np.round(v, decimals) + 0.0 if v.dtype.kind == "f" else v
            h.update(k.encode()); h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(k.encode()); h.update(np.array(sorted(v), np.int64).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("batch", [1, 64])
@pytest.mark.parametrize("q", [3, 4])
def test_decoy_points_are_the_vertices(q, batch):
    prob = co.decoy_vlp(q)
    V = co.decoy_vertices(q)
    off = _solve(prob, False, batch)
    on = _solve(prob, True, batch)
    X = _points(on)
    print("decoy-%d batch %d: %d points of the upper image with the flag off, %d with it on; LPs %d / %d; tie phase %s"
          % (q, batch, len(_points(off)), len(X), off["lps"], on["lps"], on["canonical_obj"]))
    assert off["canonical_obj"] == ZERO
    assert on["canonical_obj"]["capped"] == 0 and on["canonical_obj"]["entered"] > 0
    assert len(X) == q, X
    for v in V:
        assert np.abs(X - v).max(axis=1).min() <= 1e-9, (v, X)


def test_octahedron_is_unchanged():
    """P = I: every vertex of the feasible set is its own image, so the flag must not change the result"""
    prob = cc.octahedron_vlp()
    off, on = _solve(prob, False), _solve(prob, True)
    print("octahedron: tie phase %s, LPs %d / %d" % (on["canonical_obj"], off["lps"], on["lps"]))
    ph.assert_same(ph.canonical(on["dump"], decimals=6), ph.canonical(off["dump"], decimals=6), rtol=1e-9, atol=1e-9)


def _unpartnered(X, ref, tol):
    from scipy.spatial import cKDTree
    dist, _ = cKDTree(ref).query(X)
    return int((dist > tol).sum())


def test_covering_run_off_and_on_against_the_primal_variant():
    prob = synth.covering_vlp(40, 20, 4, 9)
    ref = _points(_solve(prob, alg="primal"))
    off, on = _solve(prob, False), _solve(prob, True)
    n_off, n_on = _unpartnered(_points(off), ref, ph.DEFAULT_TOL), _unpartnered(_points(on), ref, ph.DEFAULT_TOL)
    cs = on["canonical_obj"]
    row = dict(problem="covering_vlp(40, 20, 4, 9)", batch=64, eps=EPS, tol=ph.DEFAULT_TOL, primal_variant_vertices=len(ref),
               off=dict(unpartnered=n_off, points=len(_points(off)), lps=int(off["lps"]), steps=int(off["steps"])),
               on=dict(unpartnered=n_on, points=len(_points(on)), lps=int(on["lps"]), steps=int(on["steps"]), tie=cs,
                       tie_iters_per_lp=cs["tie_iters"] / max(1, int(on["lps"]))))
    print(json.dumps(row))
    out = os.environ.get("BSLV_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "canonical_obj.json"), "w") as f:
            json.dump([row], f, indent=1)
    assert off["canonical_obj"] == ZERO
    assert cs["entered"] > 0 and cs["capped"] == 0
    assert n_on <= n_off, "points without a partner at %g: %d with the flag on, %d with it off" % (ph.DEFAULT_TOL, n_on, n_off)


def test_environment_switch(monkeypatch):
    prob = co.decoy_vlp(3)
    plain = _solve(prob, False)
    flag = _solve(prob, True)
    monkeypatch.setenv("BSLV_CANONICAL_OBJ", "1")
    env = _solve(prob, False)
    assert _digest(ph.canonical(env["dump"], decimals=6)) == _digest(ph.canonical(flag["dump"], decimals=6))
    assert env["canonical_obj"] == flag["canonical_obj"] and env["lps"] == flag["lps"]
    monkeypatch.delenv("BSLV_CANONICAL_OBJ")
    monkeypatch.setenv("BSLV_CANONICAL_DUAL", "1")      # the primal variant's switch does not touch the dual variant
    other = _solve(prob, False)
    assert _digest(ph.canonical(other["dump"], decimals=6)) == _digest(ph.canonical(plain["dump"], decimals=6))
    assert other["canonical_obj"] == ZERO and other["lps"] == plain["lps"]


def test_revised_form_fails_with_the_lp_engines_message(monkeypatch):
    """no silent fallback: an LP engine that comes up in the revised form refuses the switch, and so does the call"""
    from bensolve_amd._lib import BslvError
    monkeypatch.setenv("BSLV_LP_REV", "1")
    prob = co.decoy_vlp(3)
    assert vlp.solve_primal(prob, eps_benson_phase2=EPS, batch=8, alg_phase2="dual")["status"] == "optimal"      # (without the flag it runs)
    with pytest.raises(BslvError, match="revised"):
        vlp.solve_primal(prob, eps_benson_phase2=EPS, batch=8, alg_phase2="dual", canonical=True)
