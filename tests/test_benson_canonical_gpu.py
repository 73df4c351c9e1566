"""GPU: the Benson driver with cuts from canonical duals (bslv_benson_set_canonical).

Known answers: the octahedron VLP (P = I on |x|_1 <= 1) has an upper image of seven facets, the hypercube VLP (P = I on [0,1]^4) the
orthant at the origin with four; their vertices lie on three and more facets, so every P2(v) the run meets near a vertex is primal
degenerate.  With the switch on EVERY cut has to be one of the facets -- not merely a supporting hyperplane -- and the final facet
set exactly those, for two batch policies and batches of 1 and 64.

Measured, not promised: covering_vlp(40, 20, 4, 9) to termination with the switch off and on against the sequential CPU oracle --
the points without a partner at poly_harness.DEFAULT_TOL must not be more with the switch on than with it off; the counts are printed
and, where BSLV_RECORD_DIR names a directory, written to canonical_dual.json there (profiles/canonical_dual_parity.txt holds the run
recorded with the feature)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import canonical_cases as cc
import poly_harness as ph
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine

pytestmark = pytest.mark.gpu
EPS = 1e-9
TOL = 1e-9


def _known(name):
    """(problem, facet normals scaled to c.w = 1, value w.y on each facet)"""
    if name == "octahedron":
        N = cc.octahedron_normals()
        return cc.octahedron_vlp(), N, -1.0 / (N > 0).sum(axis=1)
    return cc.hypercube_vlp(4), np.eye(4), np.zeros(4)


def _run_recording_cuts(prob, policy, batch, canonical):
    """to termination, one outer iteration at a time; returns (normals of all cut records, canonical dump, driver counters)"""
    q = prob["q"]
    eng = BensonEngine(prob, eps=EPS, pool_slots=4 * batch + 64)
    eng.set_policy(policy)
    if canonical:
        eng.set_canonical(1)
        assert eng.get_canonical() == 1
    assert eng.start() == 0
    cuts = []
    for _ in range(10000):
        nl, nt = eng.collect(batch)
        if nt == 0:
            break
        rec, piv, ls = eng.solve_local(nl)
        assert np.all(rec[:, 1] == 4)
        for r in rec[rec[:, 2] != 0]:
            w = np.concatenate([r[4:4 + q - 1], [1.0 - r[4:4 + q - 1].sum()]])        # c.w = 1, c = (1..1)
            cuts.append(w)
        st = eng.apply(rec)
        assert st["failed"] == 0
    else:
        raise AssertionError("the run did not end")
    eng.poly_call("dual_adjacency")
    got = ph.canonical(eng.poly_dump(), decimals=6)
    cs = eng.canonical_stats()
    eng.close()
    return np.array(cuts).reshape(-1, q), got, cs


@pytest.mark.parametrize("batch", [1, 64])
@pytest.mark.parametrize("policy", [1, 3])
@pytest.mark.parametrize("name", ["octahedron", "hypercube"])
def test_every_cut_is_a_facet(name, policy, batch):
    prob, N, val = _known(name)
    q = prob["q"]
    cuts, got, cs = _run_recording_cuts(prob, policy, batch, True)
    print("%s policy %d batch %d: %d cuts, tie phase %s" % (name, policy, batch, len(cuts), cs["total"]))
    assert len(cuts) >= len(N) - q                      # (PART 1 delivers up to q facets itself)
    for w in cuts:
        assert np.abs(N - w).max(axis=1).min() <= TOL, "cut normal %s is no facet normal" % w
    # the facets of the result (dual vertices with a live vertex on them): exactly the known ones
    Y = got["Y"][got["di"] == 0]
    assert len(Y) == len(N), (len(Y), len(N))
    W = np.hstack([Y[:, :q - 1], 1.0 - Y[:, :q - 1].sum(axis=1, keepdims=True)])
    for w, a in zip(N, val):
        d = np.abs(W - w).max(axis=1)
        k = int(d.argmin())
        assert d[k] <= TOL and abs(Y[k, q - 1] - a) <= TOL, (w, a, W[k], Y[k, q - 1])
    assert cs["total"]["capped"] == 0


def test_homogeneous_engine_refuses_the_switch(monkeypatch):
    from bensolve_amd import load_library
    lib = load_library()
    prob = cc.octahedron_vlp()
    m, n, q = prob["m"], prob["n"], prob["q"]
    f8 = lambda a: np.ascontiguousarray(a, np.float64)
    A, P, R, c, eta = f8(prob["A"]), f8(prob["P"]), f8(np.eye(q)), f8(np.ones(q)), f8(np.ones(q))
    rt, ct = np.ascontiguousarray(prob["rtype"], np.uint8), np.ascontiguousarray(prob["ctype"], np.uint8)
    rlb, rub, clb, cub = f8(prob["rlb"]), f8(prob["rub"]), f8(prob["clb"]), f8(prob["cub"])
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.bslv_benson_create_ex.argtypes = [ctypes.POINTER(vp), i, i, i] + [vp] * 8 + [vp, i, vp, vp, i, i, d, i]
    lib.bslv_benson_set_canonical.argtypes = [vp, i]
    lib.bslv_benson_get_canonical.argtypes = [vp]
    lib.bslv_benson_destroy.argtypes = [vp]
    lib.bslv_benson_destroy.restype = None
    monkeypatch.setenv("BSLV_CANONICAL_DUAL", "1")      # (the environment switch leaves a homogeneous engine alone)
    h = vp()
    rc = lib.bslv_benson_create_ex(ctypes.byref(h), m, n, q, A.ctypes.data, P.ctypes.data, rt.ctypes.data, rlb.ctypes.data, rub.ctypes.data,
                                   ct.ctypes.data, clb.ctypes.data, cub.ctypes.data, R.ctypes.data, q, c.ctypes.data, eta.ctypes.data, 1, 0, EPS, 16)
    assert rc == 0, lib.bslv_last_error().decode()
    try:
        assert lib.bslv_benson_get_canonical(h) == 0
        assert lib.bslv_benson_set_canonical(h, 1) == 2                 # BSLV_E_ARG
        assert "homogeneous" in lib.bslv_last_error().decode()
        assert lib.bslv_benson_set_canonical(h, 0) == 0
    finally:
        lib.bslv_benson_destroy(h)
    # ... and switches an inhomogeneous one on
    eng = BensonEngine(prob, eps=EPS, pool_slots=16)
    try:
        assert eng.get_canonical() == 1
    finally:
        eng.close()


# ---- measured: the covering problem behind one of the allow-listed comparisons of tests/test_benson_gpu.py ----
def _digest(can, decimals=6):
    """SHA-256 over the whole canonical dump (scripts/probe/fill_probe.py's)"""
    h = hashlib.sha256()
    for k in sorted(can):
        v = can[k]
        if isinstance(v, np.ndarray):
            a = np.round(v, decimals) + 0.0 if v.dtype.kind == "f" else v
            h.update(k.encode()); h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(k.encode()); h.update(np.array(sorted(v), np.int64).tobytes())
    return h.hexdigest()


_oracle = {}


def _oracle_result(prob):
    if "exp" not in _oracle:
        import oracle_api
        rc, fp, st = oracle_api.benson_phase2_primal(prob, eps=EPS)
        assert rc == 0
        fp.dual_adjacency()
        _oracle["exp"] = ph.canonical(fp.dump(), decimals=6)
        fp.close()
    return _oracle["exp"]


def _to_termination(prob, policy, batch, switch):
    """switch: None = the new call is never made, 0 = switched on and off again before the run, 1 = on"""
    eng = BensonEngine(prob, eps=EPS, pool_slots=4 * batch + 64)
    eng.set_policy(policy)
    if switch is not None:
        eng.set_canonical(1)
        if not switch:
            eng.set_canonical(0)
    assert eng.start() == 0
    steps = eng.run(batch)
    eng.poly_call("dual_adjacency")
    got = ph.canonical(eng.poly_dump(), decimals=6)
    tot, cs = eng.totals(), eng.canonical_stats()["total"]
    eng.close()
    return got, dict(tot, steps=steps), cs


def _mode(got, exp, tol):
    """assert_benson_results_agree's verdict without its assertion: "exact", or its own count of points without a partner"""
    nun = ph.unmatched_points(got, exp, tol)
    if got["X"].shape == exp["X"].shape and got["Y"].shape == exp["Y"].shape:
        try:
            ph.assert_same(got, exp, rtol=tol, atol=tol)
            return "exact", nun
        except AssertionError:
            pass
    return "sliver(%d)" % nun, nun


@pytest.mark.parametrize("policy", [1, 3])
def test_covering_run_off_and_on_against_the_oracle(policy):
    prob = synth.covering_vlp(40, 20, 4, 9)
    batch = 128
    exp = _oracle_result(prob)
    never, tot_never, _ = _to_termination(prob, policy, batch, None)
    off, tot_off, cs_off = _to_termination(prob, policy, batch, 0)
    on, tot_on, cs_on = _to_termination(prob, policy, batch, 1)
    # off: the run of an engine that never saw the call
    assert _digest(off) == _digest(never) and tot_off == tot_never
    assert cs_off == dict(entered=0, tie_pivots=0, no_candidate=0, capped=0)
    mode_off, n_off = _mode(off, exp, ph.DEFAULT_TOL)
    mode_on, n_on = _mode(on, exp, ph.DEFAULT_TOL)
    row = dict(problem="covering_vlp(40, 20, 4, 9)", policy=policy, batch=batch, eps=EPS, tol=ph.DEFAULT_TOL,
               off=dict(unmatched=n_off, mode=mode_off, vertices=len(off["X"]), facets=len(off["Y"]), **tot_off),
               on=dict(unmatched=n_on, mode=mode_on, vertices=len(on["X"]), facets=len(on["Y"]), tie=cs_on,
                       tie_pivots_per_lp=cs_on["tie_pivots"] / max(1, tot_on["lps"]), **tot_on),
               oracle=dict(vertices=len(exp["X"]), facets=len(exp["Y"])))
    print(json.dumps(row))
    out = os.environ.get("BSLV_RECORD_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "canonical_dual.json")
        rows = json.load(open(path)) if os.path.exists(path) else []
        rows = [r for r in rows if r.get("policy") != policy] + [row]
        with open(path, "w") as f:
            json.dump(sorted(rows, key=lambda r: r["policy"]), f, indent=1)
    assert cs_on["entered"] > 0 and cs_on["capped"] == 0
    assert n_on <= n_off, "points without a partner at %g: %d with the switch on, %d with it off" % (ph.DEFAULT_TOL, n_on, n_off)
