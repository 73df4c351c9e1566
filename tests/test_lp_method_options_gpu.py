"""GPU: the simplex method of the Benson driver's LPs (bslv_benson_set_lp_method, include/bslv_hip.h): the start LPs, every P2(v) batch
and both stages of its retry go through bslv_lpq_solve_batch_method.  S-small, 3 outer iterations of 64 LPs, tableau form; and the
refusal of a revised engine that is asked for PRIMAL together with canonical duals."""
import contextlib
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bensolve_amd import synth
from bensolve_amd._lib import BslvError
from bensolve_amd.benson import BensonEngine

pytestmark = pytest.mark.gpu

DUAL, PRIMAL, REPAIR = 0, 1, 2
BATCH, STEPS = 64, 3


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _run(method, touch=False, **env):
    """S-small for 3 steps: per step the LP engine's phase-1 counter of its last solve call, then the totals, the driver's per-method
    counts and the SHA-256 of the polyhedron (the keys tests/test_benson_gpu.py hashes)"""
    with _env(**dict(dict(BSLV_LP_REV=None, BSLV_BENSON_LP_METHOD=None, BSLV_FORCE_RETRY=None), **env)):
        eng = BensonEngine(synth.CONFIGS["S-small"](), eps=1e-7, pool_slots=4 * BATCH + 64)
        assert eng.get_lp_method() == (-1 if "BSLV_BENSON_LP_METHOD" not in env else {"dual": 0, "primal": 1, "repair": 2}[env["BSLV_BENSON_LP_METHOD"]])
        if touch:
            assert eng.set_lp_method(PRIMAL) == 0 and eng.set_lp_method(-1) == 0
        if method is not None:
            assert eng.set_lp_method(method) == 0 and eng.get_lp_method() == method
        assert eng.start() == 0
        phase1, lps = [], []
        for _ in range(STEPS):
            s = eng.step(BATCH)
            lps.append(s["lps"])
            phase1.append(eng.lp_call("last_stats")["phase1_lps"])
        tot, counts, d = eng.totals(), eng.lp_method_stats(), eng.poly_dump()
        eng.close()
    h = hashlib.sha256()
    for key in ("pu", "pi", "du", "di", "X", "Y", "E", "I"):
        h.update(np.ascontiguousarray(d[key]).tobytes())
    return dict(phase1=phase1, lps=lps, totals=tot, counts=counts, sha=h.hexdigest())


def test_primal_reaches_the_lp_engine():
    r = _run(PRIMAL)
    assert max(r["phase1"]) > 0, r          # (bslv_lpq_last_phase1_stats[0] of a P2(v) batch: LPs that entered phase 1)
    assert r["counts"][PRIMAL] >= r["totals"]["lps"] > 0 and r["counts"][DUAL] == r["counts"][REPAIR] == 0, r


def test_the_retry_keeps_the_method():
    plain, forced = _run(PRIMAL), _run(PRIMAL, BSLV_FORCE_RETRY="1")
    # every other LP of every batch is solved again (from the root tableau, stage 0 of the retry): under PRIMAL too, and under nothing else
    assert plain["counts"][PRIMAL] >= plain["totals"]["lps"] > 0, plain
    assert forced["counts"][PRIMAL] - forced["totals"]["lps"] >= sum(n // 2 for n in forced["lps"]) > 0, forced
    assert forced["counts"][DUAL] == forced["counts"][REPAIR] == 0, forced
    # ... and on the engine's side: the last solve call of a step is then its retry batch, and it entered phase 1 -- which only a
    # PRIMAL (or REPAIR) call has (bslv_lpq_last_phase1_stats[0]; a DUAL call reads 0)
    assert max(forced["phase1"]) > 0, forced


def test_unset_is_the_trajectory_it_always_was():
    """unset: bslv_lpq_solve_batch, nothing else.  DUAL through the per-call method is that call bit for bit in the tableau form (the
    engine's own method is DUAL), so the three runs have to end in the same polyhedron, with the same LPs and pivots"""
    unset, touched, dual, env = _run(None), _run(None, touch=True), _run(DUAL), _run(None, BSLV_BENSON_LP_METHOD="dual")
    assert unset["counts"] == [0, 0, 0] == touched["counts"]
    assert dual["counts"][DUAL] >= dual["totals"]["lps"] > 0 and env["counts"] == dual["counts"]
    for other in (touched, dual, env):
        assert (other["sha"], other["totals"], other["lps"]) == (unset["sha"], unset["totals"], unset["lps"]), (unset, other)


def test_bad_methods_are_refused():
    with _env(BSLV_LP_REV=None):
        eng = BensonEngine(synth.covering_vlp(30, 15, 3, 5), eps=1e-7, pool_slots=128)
        assert eng.set_lp_method(3) != 0 and eng.set_lp_method(-2) != 0 and eng.get_lp_method() == -1
        eng.close()


def test_revised_engine_refuses_primal_with_the_canonical_call():
    with _env(BSLV_LP_REV="1", BSLV_BENSON_LP_METHOD=None):
        eng = BensonEngine(synth.covering_vlp(30, 15, 3, 5), eps=1e-7, pool_slots=128)
        eng.lib.bslv_lpq_is_revised.argtypes = [__import__("ctypes").c_void_p]
        assert eng.lib.bslv_lpq_is_revised(eng._lp_h) == 1
        eng.set_canonical(1)
        assert eng.set_lp_method(PRIMAL) == 0
        assert eng.start() == 0          # (the weighted-sum LPs of the start are not canonical calls)
        with pytest.raises(BslvError) as e:
            eng.step(32)
        assert "bslv_benson_set_lp_method" in str(e.value) and "bslv_benson_set_canonical" in str(e.value), str(e.value)
        eng.close()
        eng = BensonEngine(synth.covering_vlp(30, 15, 3, 5), eps=1e-7, pool_slots=128)
        eng.set_canonical(1)
        assert eng.set_lp_method(DUAL) == 0 and eng.start() == 0
        s = eng.step(32)                 # DUAL is the canonical call's own method: accepted
        assert s["lps"] > 0 and eng.lp_method_stats()[DUAL] >= s["lps"]
        eng.close()


# ---- the phases: lp_methods of vlp.solve_primal (both phase-2 algorithms) ------------------------------------------------------------
import json
import subprocess

from bensolve_amd.vlp import solve_primal

EXDIR = os.path.join(ROOT, "tests", "golden", "ex")
TRIPLES = [("primal", "primal", "primal"), ("dual", "dual", "dual"), ("repair", "repair", "repair")]
PT = dict(phase0=0, phase1_primal=1, phase1_dual=2, phase2_primal=3, phase2_dual=4)      # the reference's phase_type


def _problem(name):
    if name.startswith("ex"):
        return synth.read_vlp(os.path.join(EXDIR, name + ".vlp"))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import vlp_general_cases as vg
    return vg.unbounded_general(14, 10, 3, 5)      # a generated general VLP with an unbounded upper image: all three phases run


def _solve(name, alg2, triple):
    prob = _problem(name)
    with _env(BSLV_LP_REV=None, BSLV_BENSON_LP_METHOD=None, BSLV_LP_METHOD=None):
        return solve_primal(prob, cone_kind=prob.get("cone_kind", 0), gen=prob.get("gen"), c=prob["c"] if prob.get("c") is not None and np.any(prob["c"]) else None,
                            batch=16, alg_phase2=alg2, lp_methods=triple)


_BASE = {}


def _base(name, alg2):
    if (name, alg2) not in _BASE:
        _BASE[(name, alg2)] = _solve(name, alg2, None)
    return _BASE[(name, alg2)]


@pytest.mark.parametrize("triple", TRIPLES, ids=[t[0] for t in TRIPLES])
@pytest.mark.parametrize("alg2", ["primal", "dual"])
@pytest.mark.parametrize("name", ["ex01", "ex05", "ex06", "general"])
def test_every_phase_runs_under_the_asked_method(name, alg2, triple):
    import poly_harness as ph
    base, got = _base(name, alg2), _solve(name, alg2, triple)
    assert base["status"] == "optimal" and base["lp_method_stats"] == [[0, 0, 0]] * 5, (base["status"], base["lp_method_stats"])
    assert got["status"] == "optimal", (name, alg2, triple, got["status"], got["message"])
    # the images: every vertex and direction of either run has a partner within 1e-6 in the other (the tolerance of the project's
    # end-to-end comparisons of two cut orders, poly_harness.assert_benson_results_agree): mutual containment, and more
    ca, cb = ph.canonical(got["dump"], decimals=6), ph.canonical(base["dump"], decimals=6)
    assert ph.unmatched_points(ca, cb, 1e-6) == 0, (name, alg2, triple, len(ca["X"]), len(cb["X"]))
    # every LP of every phase that ran under the asked method, none under another
    m = LP_M[triple[0]]
    stats = got["lp_method_stats"]
    for p in range(5):
        assert all(stats[p][k] == 0 for k in range(3) if k != m), (name, alg2, triple, stats)
    assert stats[PT["phase0"]][m] > 0 and stats[PT["phase1_primal"]][m] > 0 and stats[PT["phase1_dual"]][m] == 0, stats
    assert stats[PT["phase2_" + alg2]][m] > 0 and stats[PT["phase2_" + ("dual" if alg2 == "primal" else "primal")]][m] == 0, stats


LP_M = dict(dual=0, primal=1, repair=2)


@pytest.mark.parametrize("triple", TRIPLES, ids=[t[0] for t in TRIPLES])
@pytest.mark.parametrize("name,status", [("ex02", "infeasible"), ("ex03", "no vertex"), ("ex04", "unbounded")])
def test_documented_outcomes_stay_under_every_triple(name, status, triple):
    """ex/example02.m, 03, 04: infeasible (phase 2 part 1), no vertex and totally unbounded (phase 0)"""
    base, got = _base(name, "primal"), _solve(name, "primal", triple)
    assert base["status"] == status and got["status"] == status and got["message"] == base["message"], (base["status"], got["status"], got["message"])


def test_phase1_dual_takes_the_method_of_phase_1():
    prob = _problem("ex01")
    with _env(BSLV_LP_REV=None):
        got = solve_primal(prob, batch=16, alg_phase1="dual", lp_methods=(None, "repair", None))
    assert got["status"] == "optimal"
    stats = got["lp_method_stats"]
    assert stats[PT["phase1_dual"]][2] > 0 and sum(map(sum, stats)) == stats[PT["phase1_dual"]][2], stats


# ---- the command line: off as shipped --------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hybrid.npz"))
OUTPUTS = ("_img_p.sol", "_img_d.sol", "_adj_p.sol", "_adj_d.sol", "_inc_p.sol", "_inc_d.sol", "_c.sol")


def _cli(tmp_path, tag, extra, switch):
    from test_cli_gpu import read_img
    d = os.path.join(tmp_path, tag)
    os.makedirs(d)
    base = os.path.join(d, "ex01")
    env = dict(os.environ)
    for k in ("BSLV_LP_METHOD_OPTIONS", "BSLV_LP_REV", "BSLV_LP_METHOD"):
        env.pop(k, None)
    if switch:
        env["BSLV_LP_METHOD_OPTIONS"] = "1"
    r = subprocess.run([CLI, os.path.join(EXDIR, "ex01.vlp"), "-a", "dual", "-o", base] + extra, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    files = {s: open(base + s, "rb").read() for s in OUTPUTS if os.path.exists(base + s)}
    return base, files, open(base + ".log").read(), read_img


def test_cli_hands_the_methods_on_only_with_the_switch(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_cli_gpu import _gold_rows, EX_TOL
    opts = ["-l", "dual_simplex", "-k", "primal_simplex"]
    base, files, log, read_img = _cli(tmp_path, "on", opts, True)
    lines = {l.split(":")[0].strip(): l.split(":", 1)[1].strip() for l in log.splitlines() if l.strip().startswith("lp_method_lps_")}
    assert set(lines) == {"lp_method_lps_" + p for p in PT}, log
    cnt = {k: [int(x.split()[0]) for x in v.split(",")] for k, v in lines.items()}          # dual, primal, repair
    assert cnt["lp_method_lps_phase0"][1] > 0 and cnt["lp_method_lps_phase0"][0] == cnt["lp_method_lps_phase0"][2] == 0, log
    assert cnt["lp_method_lps_phase2_dual"][0] > 0 and cnt["lp_method_lps_phase2_dual"][1] == cnt["lp_method_lps_phase2_dual"][2] == 0, log
    assert cnt["lp_method_lps_phase1_primal"] == cnt["lp_method_lps_phase1_dual"] == cnt["lp_method_lps_phase2_primal"] == [0, 0, 0], log
    t, X, _ = read_img(base + "_img_p.sol")
    gt, gX = _gold_rows(GOLD["ex01/p_type"], GOLD["ex01/p"])
    assert np.array_equal(t, gt)
    np.testing.assert_allclose(X, gX, rtol=EX_TOL, atol=EX_TOL)
    # without the variable: the same command is the run without -l / -k, byte for byte, apart from the option lines of the .log
    _, off, log_off, _ = _cli(tmp_path, "off", opts, False)
    _, plain, log_plain, _ = _cli(tmp_path, "plain", [], False)
    assert off == plain and set(off) == set(OUTPUTS), (sorted(off), sorted(plain))
    strip = lambda s, d: [l for l in s.replace(os.path.join(tmp_path, d), "").splitlines() if "lp_method_phase" not in l and "CPU time" not in l]
    assert strip(log_off, "off") == strip(log_plain, "plain")
    assert "lp_method_lps_" not in log_off


# ---- the reference's driver on the compat layer ---------------------------------------------------------------------------------------------
def test_reference_driver_on_the_compat_layer_with_the_switch(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_lp_compat_gpu as tc
    if not os.path.exists(tc.EXE):
        pytest.skip("oracle/_ref is built only where the reference's sources are")
    base = os.path.join(tmp_path, "ex01")
    env = dict(os.environ, BSLV_LP_METHOD_OPTIONS="1")
    r = subprocess.run([tc.EXE, os.path.join(EXDIR, "ex01.vlp"), "-m", "0", "-o", base], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for side in ("p", "d"):
        t, X = tc.rows(base + "_img_%s.sol" % side)
        gt, gX = tc.gold_rows(tc.GOLD["ex01/%s_type" % side], tc.GOLD["ex01/%s" % side])
        assert np.array_equal(t, gt), side
        np.testing.assert_allclose(X, gX, rtol=tc.EX_TOL, atol=tc.EX_TOL)
