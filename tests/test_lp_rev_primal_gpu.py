"""GPU: the primal phase 1 of the REVISED LP form and the simplex method per call (bslv_lpq_solve_batch_method: k_select_p1_rev and
phase1_prepare<true> in bensolve_amd/csrc/lp_engine.hip), against the CPU yardsticks the project already has -- the oracle's primal
simplex (oracle/lp_dense.c primal_simplex) and HiGHS -- never against the engine itself.  Optimal values: lp_cases.RTOL = 1e-9
relative, atol 1e-9 (the project's bound for primal steps against the oracle); statuses equal; check_optimality_conditions and,
where named, the device certificate (bslv_lpq_certify).

The revised form is forced with BSLV_LP_REV=1 at create and asserted with bslv_lpq_is_revised (test_lp_general_gpu._engine).  The
LP sets are the ones whose seeds were chosen on the CPU so that both yardsticks agree on every LP: the sets of
tests/test_lp_primal_gpu.py at (6, 5), (17, 23), (40, 70) and lp_cases.general_set at the revised form's launch thresholds
(33, 257) one slice of 256 threads, (24, 1536) one slice of NT_BIG threads, (24, 2049) two slices, (24, 4100) three slices with
helper workgroups.  In all 16 LPs of both arrangements of those general sets the standard basis is primal infeasible: a cold
PRIMAL start has phase-1 work in every one.  Every test first asserts that the yardsticks agree, then looks at the engine.

Run as a program: `python tests/test_lp_rev_primal_gpu.py helpers` runs the (24, 4100) cold batch of arrangement "a" and prints a
SHA-256 of everything it got (the helper-count test starts it that way); `... fill` solves the (17, 23) cold-start set and prints
statuses and objective bits as one JSON line (the poisoned-allocation test, once per fill byte)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lp_cases as lc
import lp_ray_cases as rc
from lp_cases import RTOL, NLP, BAD, check_optimality_conditions, oracle_primal
from lp_ray_cases import NONE as K_NONE, FARKAS, DIRECTION
from test_lp_general_gpu import _engine, _same_bits
from test_lp_primal_gpu import lp_set, references, boxed_model, cold_solve, _row_range_engine
from test_lp_ray_gpu import _compare

pytestmark = pytest.mark.gpu

DUAL, PRIMAL, REPAIR = 0, 1, 2
OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED = 4, 0, 1, 3
DANTZIG, DEVEX = 0, 1
E_ARG = 2
NONE = np.zeros((1, 0))
SMALL = [(6, 5), (17, 23), (40, 70)]
EDGES = [(33, 257), (24, 1536), (24, 2049), (24, 4100)]
KEYS = ("st", "it", "obj", "prim", "dual")


def _read(eng, dst, st, it):
    n = eng.M + eng.N
    return dict(st=np.array(st, np.int32), it=np.array(it, np.int32), obj=eng.obj(dst), prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n))


def _assert_bits(a, b, tag, keys=KEYS):
    for k in keys:
        assert _same_bits(a[k], b[k]), (tag, k, a[k], b[k])


def _counters(stats):
    """last_stats without the two clocks"""
    return {k: v for k, v in stats.items() if not k.endswith("_ms")}


# ---- the small sets, one LP per engine, cold and in place (shared by the tests 1, 7 and 10) ---------------------------------------
_SMALL = {}


def cold_set_rev(M, N, period=0):
    """every LP of the set of test_lp_primal_gpu.lp_set(M, N) from a reset slot of a revised engine under PRIMAL, once"""
    key = (M, N, period)
    if key not in _SMALL:
        rows = []
        for A, lo, up, cost in lp_set(M, N):
            eng = _engine(A, lo, up, cost, 0, 0, 2, "revised")
            if period:
                assert eng.set_refactor_period(period) == 0
            eng.reset_slot(0)
            st, it = eng.solve_batch_method(PRIMAL, [0], [0], NONE, NONE)
            rows.append(dict(st=int(st[0]), iters=int(it[0]), obj=float(eng.obj([0])[0]), prim=eng.primal([0], 0, M + N)[0], dual=eng.dual([0], 0, M + N)[0],
                             stats=eng.last_stats(), period=eng.last_period_stats()))
            eng.close()
        _SMALL[key] = rows
    return _SMALL[key]


# ---- 1. cold start under PRIMAL, small shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SMALL)
def test_cold_start_under_primal_small_shapes(oracle, M, N):
    ref = references(M, N)
    assert ref[0]["st"] == INFEASIBLE and ref[1]["st"] == UNBOUNDED                 # the two built on purpose
    for t, r in enumerate(ref):
        assert r["st"] == r["st_highs"], (t, r["st"], r["st_highs"])                # (the yardsticks agree)
    p1_lps = p1_its = 0
    for t, (r, got) in enumerate(zip(ref, cold_set_rev(M, N))):
        print("lp %d: status %d (oracle %d) iters %d obj %r (oracle %r) phase 1: %s" % (t, got["st"], r["st"], got["iters"], got["obj"], r["obj"],
              {k: v for k, v in got["stats"].items() if k.startswith("phase1")}))
        assert got["st"] == r["st"], (t, got["st"], r["st"])
        p1_lps += got["stats"]["phase1_lps"]
        p1_its += got["stats"]["phase1_iterations"]
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(got["obj"], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
            np.testing.assert_allclose(got["obj"], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
            check_optimality_conditions(r["A"], r["lo"], r["up"], r["cost"], got["obj"], got["prim"], got["dual"], (M, N, t))
    assert p1_lps > 0 and p1_its > 0, (p1_lps, p1_its)


# ---- 2. cold start under PRIMAL at the launch thresholds: 16 LPs, one lock-step batch from 16 reset slots in place -----------------
_COLD = {}


def cold_batch(M, N, arr):
    key = (M, N, arr)
    if key not in _COLD:
        s = lc.general_set(M, N, arr)
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], NLP, "revised")
        dst = np.arange(NLP, dtype=np.int32)
        for k in dst:
            eng.reset_slot(int(k))
        st, it = eng.solve_batch_method(PRIMAL, dst, dst, s["vlo"], s["vup"])
        rec = _read(eng, dst, st, it)
        rec["stats"] = eng.last_stats()
        rec["verdict"] = eng.certify(dst, s["vlo"], s["vup"])["verdict"]
        eng.close()
        _COLD[key] = rec
    return _COLD[key]


def _digest(rec):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(rec[k]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", EDGES)
def test_cold_batch_under_primal_at_the_launch_thresholds(oracle, M, N, arr):
    ref, _ = lc.assert_references_agree(M, N, arr)          # (LP BAD INFEASIBLE, at least 12 OPTIMAL, both yardsticks agree)
    rec = cold_batch(M, N, arr)
    print("cold PRIMAL batch (%d, %d) %s: statuses %s pivots %s %s" % (M, N, arr, rec["st"], rec["it"], _counters(rec["stats"])))
    assert not np.any(rec["st"] == UNDEFINED), rec["st"]      # (a retry from a reset slot would be the same solve)
    assert np.array_equal(rec["st"], [r["st"] for r in ref]), (rec["st"], [r["st"] for r in ref])
    assert rec["stats"]["phase1_lps"] == NLP and rec["stats"]["phase1_iterations"] > 0, rec["stats"]
    for t, r in enumerate(ref):
        if r["st"] != OPTIMAL:
            continue
        np.testing.assert_allclose(rec["obj"][t], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
        np.testing.assert_allclose(rec["obj"][t], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
        assert rec["verdict"][t] == 0, (t, rec["verdict"])


# ---- 3. batch against alone ------------------------------------------------------------------------------------------------------------
def test_cold_batch_equals_its_lps_alone(oracle):
    M, N, arr = 24, 2049, "a"
    lc.assert_references_agree(M, N, arr)
    together = cold_batch(M, N, arr)
    s = lc.general_set(M, N, arr)
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], NLP, "revised")
    st, it = [], []
    for b in range(NLP):
        eng.reset_slot(b)
        s1, i1 = eng.solve_batch_method(PRIMAL, [b], [b], s["vlo"][b:b + 1], s["vup"][b:b + 1])
        st.append(s1[0]); it.append(i1[0])
    alone = _read(eng, np.arange(NLP, dtype=np.int32), st, it)
    eng.close()
    _assert_bits(together, alone, "16 together against 16 alone")


# ---- 4. helpers do not show ------------------------------------------------------------------------------------------------------------
def _child_helpers():
    rec = cold_batch(24, 4100, "a")
    print("helpers %s statuses %s" % (os.environ.get("BSLV_REV_HELPERS"), "".join(str(v) for v in rec["st"])))
    print("sha256 " + _digest(rec))


def test_cold_batch_does_not_depend_on_the_number_of_helpers(oracle):
    ref, _ = lc.assert_references_agree(24, 4100, "a")
    out = []
    for helpers in ("1", None):
        env = dict(os.environ)
        env.pop("BSLV_REV_HELPERS", None)
        if helpers:
            env["BSLV_REV_HELPERS"] = helpers
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "helpers"], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, "helpers %s: rc %d\n%s" % (helpers, p.returncode, p.stderr[-1500:])      # (the first child that fails ends the test)
        lines = p.stdout.strip().splitlines()
        print(lines[-2])
        assert lines[-2].split()[3] == "".join(str(r["st"]) for r in ref), lines[-2]
        out.append(lines[-1])
    assert out[0].startswith("sha256 ") and out[0] == out[1], out


# ---- 5. a warm start that is infeasible on both sides -----------------------------------------------------------------------------------
def test_warm_start_infeasible_on_both_sides(oracle):
    M, N = 17, 23
    A, lo, up, cost = boxed_model(M, N, 202)
    eng = _engine(A, lo, up, cost, 0, 0, 4, "revised")
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], NONE, NONE)
    assert st[0] == OPTIMAL
    prim, dual = eng.primal([0], 0, M + N)[0], eng.dual([0], 0, M + N)[0]
    # (the search of test_lp_primal_gpu.test_warm_start_infeasible_on_both_sides: a nonbasic row loses the bound under its reduced cost,
    # a basic variable gets an upper bound below its value; of the pairs on offer, the first whose LP the oracle solves to optimality)
    nonbasic = [k for k in range(M) if abs(dual[k]) > 1e-3]
    basic = [k for k in range(M + N) if dual[k] == 0.0 and prim[k] - lo[k] > 1.0 and up[k] - prim[k] > 1e-6]
    assert nonbasic and basic
    chosen = None
    for kn in nonbasic:
        for kb in basic:
            lo2, up2 = lo.copy(), up.copy()
            if dual[kn] > 0: lo2[kn] = -np.inf
            else: up2[kn] = np.inf
            up2[kb] = prim[kb] - 0.5
            so, zo = oracle_primal(A, lo2, up2, cost)
            if so == OPTIMAL:
                chosen = (lo2, up2, zo)
                break
        if chosen:
            break
    assert chosen, "no pair of changes leaves a solvable LP"
    lo2, up2, zo = chosen
    eng.set_bounds(lo2, up2)
    st, _ = eng.solve_batch([0], [1], NONE, NONE)
    assert st[0] == UNDEFINED                       # the default: the dual simplex cannot start there
    for method, dst in ((REPAIR, 2), (PRIMAL, 3)):
        st, it = eng.solve_batch_method(method, [0], [dst], NONE, NONE)
        stats = eng.last_stats()
        z = eng.obj([dst])[0]
        print("method %d: status %d iters %d obj %r (oracle %r) %s" % (method, st[0], it[0], z, zo, _counters(stats)))
        assert st[0] == OPTIMAL, (method, st)
        np.testing.assert_allclose(z, zo, rtol=RTOL, atol=1e-9)
        assert stats["phase1_lps"] == 1, stats
        check_optimality_conditions(A, lo2, up2, cost, z, eng.primal([dst], 0, M + N)[0], eng.dual([dst], 0, M + N)[0], method)
        assert eng.get_method() == DUAL
    eng.close()


# ---- 6. a mixed batch under REPAIR ------------------------------------------------------------------------------------------------------
def _row_range_engine_rev(seed, slots):
    """test_lp_primal_gpu._row_range_engine in the revised form: the boxed model with per-LP bounds on all its rows, slot 0 solved"""
    M, N = 17, 23
    A, lo, up, cost = boxed_model(M, N, seed)
    eng = _engine(A, lo, up, cost, 0, M, slots, "revised")
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], lo[None, :M], up[None, :M])
    assert st[0] == OPTIMAL
    return eng, M, N, lo, up


def _mixed_bounds(eng, M, lo, up, B):
    """the batch of test_lp_primal_gpu.test_mixed_batch_under_repair_equals_its_lps_alone: other boxes for every LP (the dual simplex
    starts), and for every second LP a bound gone from under a reduced cost (it cannot)"""
    dual = eng.dual([0], 0, M)[0]
    nonbasic = [k for k in range(M) if abs(dual[k]) > 1e-3]
    assert nonbasic
    rng = np.random.default_rng(5)
    vlo, vup = np.tile(lo[:M], (B, 1)), np.tile(up[:M], (B, 1))
    for b in range(B):
        vlo[b] -= rng.integers(0, 2, size=M); vup[b] += rng.integers(0, 2, size=M)
        if b % 2:
            k = nonbasic[(b // 2) % len(nonbasic)]
            if dual[k] > 0: vlo[b, k] = -np.inf
            else: vup[b, k] = np.inf
    return vlo, vup


def test_mixed_batch_under_repair_equals_its_lps_alone():
    B = 16
    eng, M, N, lo, up = _row_range_engine_rev(303, 2 * B + 1)
    vlo, vup = _mixed_bounds(eng, M, lo, up, B)
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch_method(REPAIR, np.zeros(B, np.int32), dst, vlo, vup)
    stats = eng.last_stats()
    print("batch: statuses %s iters %s %s" % (st, it, _counters(stats)))
    assert 0 < stats["phase1_lps"] < B, stats       # some need phase 1, some none
    assert np.all(st != UNDEFINED), st              # a result, not a retry
    together = _read(eng, dst, st, it)
    alone = dict(st=[], it=[])
    dst1 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    for b in range(B):
        s1, i1 = eng.solve_batch_method(REPAIR, [0], [dst1[b]], vlo[b:b + 1], vup[b:b + 1])
        alone["st"].append(s1[0]); alone["it"].append(i1[0])
    _assert_bits(together, _read(eng, dst1, alone["st"], alone["it"]), "batch against single LPs")
    eng.close()


# ---- 7. phase 1 across a refactorisation ------------------------------------------------------------------------------------------------
def test_phase1_across_a_periodic_refactorisation(oracle):
    M, N, K = 17, 23, 6
    ref = references(M, N)
    for r in ref:
        assert r["st"] == r["st_highs"]
    # the condition on the input, on the form that had a phase 1 all along: some LP of the set spends more than K iterations in it
    tab = [cold_solve(r["A"], r["lo"], r["up"], r["cost"], PRIMAL)["stats"]["phase1_iterations"] for r in ref]
    assert max(tab) > K, tab
    plain, per = cold_set_rev(M, N), cold_set_rev(M, N, period=K)
    print("phase-1 iterations: tableau %s\n   revised %s\n   revised, period %d %s" % (tab, [g["stats"]["phase1_iterations"] for g in plain], K, [g["stats"]["phase1_iterations"] for g in per]))
    assert max(g["stats"]["phase1_iterations"] for g in per) > K
    assert sum(g["period"]["in_rounds"] for g in per) > 0, [g["period"] for g in per]
    for t, (r, a, b) in enumerate(zip(ref, plain, per)):
        assert b["st"] == a["st"] == r["st"], (t, b["st"], a["st"], r["st"])
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(b["obj"], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
            np.testing.assert_allclose(b["obj"], a["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d (no period)" % t)


# ---- 8. rays -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_rays_of_phase1_and_of_the_primal_step(oracle, form):
    """LP 0 of the (17, 23) set (two rows with the same coefficients and contradicting bounds) and LP 1 (a free column with a cost and no
    row) under PRIMAL: what tests/test_lp_ray_gpu.py asserts of the tableau form's phase 1 -- the kind, the device certificate equal to the
    yardstick's on the same vector (_compare), verdict 0 -- in both forms through the same call; the tableau arm is the control."""
    M, N = 17, 23
    ref = references(M, N)
    assert ref[0]["st"] == ref[0]["st_highs"] == INFEASIBLE and ref[1]["st"] == ref[1]["st_highs"] == UNBOUNDED
    for t, st_want, kind_want in ((0, INFEASIBLE, FARKAS), (1, UNBOUNDED, DIRECTION)):
        r = ref[t]
        eng = _engine(r["A"], r["lo"], r["up"], r["cost"], 0, 0, 2, form)
        try:
            assert eng.set_rays(1) == 0
            eng.reset_slot(0)
            st, _ = eng.solve_batch_method(PRIMAL, [0], [0], NONE, NONE)
            assert st[0] == st_want, (form, t, st)
            rs = eng.last_ray_stats()
            assert rs == dict(farkas=int(kind_want == FARKAS), direction=int(kind_want == DIRECTION), none=0), rs
            out = eng.certify_rays([0])
            cvec = np.concatenate([np.zeros(M), r["cost"][1:]])
            kinds, rays, host = _compare(eng, r["A"], [0], lambda b: (r["lo"], r["up"]), lambda b: cvec, out, (form, "lp", t))
            print("lp %d %s: kind %d verdict %d res %s at %s" % (t, form, kinds[0], out["verdict"][0], out["res"][0].tolist(), out["at"][0].tolist()))
            assert kinds[0] == kind_want and out["verdict"][0] == 0, (form, t, kinds, out)
            assert np.abs(rays[0]).max() == 1.0
        finally:
            eng.close()


def test_unbounded_model_dual_stores_nothing_primal_a_direction():
    """test_lp_ray_gpu.test_unbounded_model_dual_stores_nothing_primal_a_direction in the revised form, the re-solve through the call"""
    M, N = 33, 257
    A, lo, up, cost = lc.unbounded_model(M, N)
    assert oracle_primal(A, lo, up, cost)[0] == UNBOUNDED and lc.highs(A, lo, up, cost)[0] == UNBOUNDED
    eng = _engine(A, lo, up, cost, 0, 0, 2, "revised")
    try:
        assert eng.set_rays(1) == 0
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [1], NONE, NONE)
        assert st[0] == UNBOUNDED, st               # (what the tableau form does on it: UNBOUNDED on the artificial bound, nothing stored)
        assert eng.last_ray_stats()["none"] >= 1 and eng.last_ray_stats()["direction"] == 0
        kind, ray = eng.get_ray([1])
        out = eng.certify_rays([1])
        assert kind[0] == K_NONE and not ray.any() and out["verdict"][0] & 8, (kind, out)
        eng.reset_slot(0)
        st, _ = eng.solve_batch_method(PRIMAL, [0], [1], NONE, NONE)
        assert st[0] == UNBOUNDED, st
        assert eng.last_ray_stats()["direction"] == 1
        out = eng.certify_rays([1])
        cvec = np.concatenate([np.zeros(M), cost[1:]])
        kinds, rays, host = _compare(eng, A, [1], lambda b: (lo, up), lambda b: cvec, out, ("unbounded model", M, N))
        print("unbounded model M %d N %d under PRIMAL, revised: res %s" % (M, N, out["res"][0].tolist()))
        assert kinds[0] == DIRECTION and out["verdict"][0] == 0, (kinds, out)
    finally:
        eng.close()


# ---- 9. nothing else moved ------------------------------------------------------------------------------------------------------------
def test_set_method_is_refused_as_before_and_get_method_stays_dual():
    eng, M, N, lo, up = _row_range_engine_rev(303, 3)
    assert eng.set_method(PRIMAL) == E_ARG and eng.set_method(REPAIR) == E_ARG and eng.get_method() == DUAL
    st, _ = eng.solve_batch_method(PRIMAL, [0], [1], lo[None, :M], up[None, :M])
    assert st[0] == OPTIMAL and eng.get_method() == DUAL
    assert eng.set_method(PRIMAL) == E_ARG and eng.get_method() == DUAL
    eng.close()


def _dual_batch_bounds(M, lo, up, B):
    rng = np.random.default_rng(11)
    return np.tile(lo[:M], (B, 1)) - rng.integers(0, 3, size=(B, M)), np.tile(up[:M], (B, 1)) + rng.integers(0, 3, size=(B, M))


def test_a_detour_through_the_call_leaves_no_trace():
    """the frame of test_lp_primal_gpu.test_default_method_is_dual_and_a_detour_leaves_no_trace, in the revised form"""
    B = 12
    out = []
    for detour in (False, True):
        eng, M, N, lo, up = _row_range_engine_rev(303, 2 * B + 2)
        if detour:
            st, _ = eng.solve_batch_method(PRIMAL, [0], [2 * B + 1], lo[None, :M], up[None, :M])       # a solve in another slot
            assert st[0] == OPTIMAL and eng.get_method() == DUAL
        vlo, vup = _dual_batch_bounds(M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        st, it = eng.solve_batch(np.zeros(B, np.int32), dst, vlo, vup)
        assert np.all(st == OPTIMAL) and eng.last_stats()["phase1_lps"] == 0
        rec = _read(eng, dst, st, it)
        rec["stats"] = _counters(eng.last_stats())
        out.append(rec)
        eng.close()
    _assert_bits(out[0], out[1], "fresh engine against one after a detour through PRIMAL")
    assert out[0]["stats"] == out[1]["stats"], (out[0]["stats"], out[1]["stats"])


@pytest.mark.parametrize("method", [DUAL, PRIMAL, REPAIR])
def test_tableau_form_the_call_is_set_method_and_solve_batch(method):
    """two twin engines of the tableau form, the mixed batch of test 6: the call against set_method + solve_batch, statistics included"""
    B = 16
    out = []
    for by_call in (True, False):
        eng, M, N, lo, up = _row_range_engine(303, B + 1)
        vlo, vup = _mixed_bounds(eng, M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        src = np.zeros(B, np.int32)
        if by_call:
            st, it = eng.solve_batch_method(method, src, dst, vlo, vup)
            assert eng.get_method() == DUAL
        else:
            assert eng.set_method(method) == 0
            st, it = eng.solve_batch(src, dst, vlo, vup)
            assert eng.set_method(DUAL) == 0
        rec = _read(eng, dst, st, it)
        rec["stats"] = _counters(eng.last_stats())
        rec["more"] = (eng.last_pricing_stats(), eng.last_primal_pricing_stats(), eng.last_ray_stats() if eng.get_rays() else None)
        out.append(rec)
        eng.close()
    print("method %d: statuses %s %s" % (method, out[0]["st"], out[0]["stats"]))
    if method == DUAL:
        assert np.any(out[0]["st"] == UNDEFINED)          # (the LPs that lost a bound: the batch is the mixed one)
    else:
        assert out[0]["stats"]["phase1_lps"] > 0
    _assert_bits(out[0], out[1], ("the call against set_method + solve_batch", method))
    assert out[0]["stats"] == out[1]["stats"] and out[0]["more"] == out[1]["more"], (out[0]["stats"], out[1]["stats"])


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_a_method_out_of_range_is_refused_and_changes_nothing(form):
    B = 12
    out = []
    for refused in (False, True):
        eng, M, N, lo, up = (_row_range_engine_rev if form == "revised" else _row_range_engine)(303, B + 1)
        vlo, vup = _dual_batch_bounds(M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        src = np.zeros(B, np.int32)
        if refused:
            st = np.full(B, -7, np.int32)
            it = np.full(B, -7, np.int32)
            eng.lib.bslv_lpq_solve_batch_method.argtypes = [__import__("ctypes").c_void_p, __import__("ctypes").c_int, __import__("ctypes").c_int] + [__import__("ctypes").c_void_p] * 6
            for bad in (7, -1):
                assert eng.lib.bslv_lpq_solve_batch_method(eng.h, bad, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data, st.ctypes.data, it.ctypes.data) == E_ARG
            assert eng.lib.bslv_lpq_solve_batch_method(None, PRIMAL, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data, st.ctypes.data, it.ctypes.data) == E_ARG
            assert np.all(st == -7) and np.all(it == -7) and eng.get_method() == DUAL
        st, it = eng.solve_batch(src, dst, vlo, vup)
        rec = _read(eng, dst, st, it)
        rec["stats"] = _counters(eng.last_stats())
        out.append(rec)
        eng.close()
    _assert_bits(out[0], out[1], "the next solve after a refused call")
    assert out[0]["stats"] == out[1]["stats"]


def test_the_pricing_switches_do_not_reach_the_revised_phase1():
    B = 12
    out = []
    for devex in (False, True):
        eng, M, N, lo, up = _row_range_engine_rev(303, B + 1)
        if devex:
            assert eng.set_pricing(DEVEX) == 0 and eng.set_primal_pricing(DEVEX) == 0
        vlo, vup = _dual_batch_bounds(M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        st, it = eng.solve_batch_method(PRIMAL, np.zeros(B, np.int32), dst, vlo, vup)
        assert np.all(st == OPTIMAL), st
        assert eng.last_pricing_stats() == dict(weighted=0, other_row=0, resets=0), eng.last_pricing_stats()
        assert eng.last_primal_pricing_stats() == dict(weighted=0, other_col=0, resets=0), eng.last_primal_pricing_stats()
        rec = _read(eng, dst, st, it)
        rec["stats"] = _counters(eng.last_stats())
        out.append(rec)
        eng.close()
    _assert_bits(out[0], out[1], "both Devex switches on against off")
    assert out[0]["stats"] == out[1]["stats"], (out[0]["stats"], out[1]["stats"])


# ---- 10. poisoned allocations ------------------------------------------------------------------------------------------------------------
def _child_fill():
    rows = [[g["st"], g["obj"].hex() if g["st"] == OPTIMAL else None] for g in cold_set_rev(17, 23)]
    print(json.dumps(dict(fill=os.environ.get("BSLV_FILL"), rows=rows)))


def test_cold_start_does_not_depend_on_the_fill_byte():
    out = []
    for fill in ("0x00", "0x7F"):
        env = dict(os.environ, BSLV_FILL=fill)
        env.pop("BSLV_ALLOC_LOG", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "fill"], env=env, capture_output=True, text=True, timeout=300)
        assert "Memory access fault" not in p.stderr, "fill %s: %s" % (fill, p.stderr[-800:])
        assert p.returncode == 0, "fill %s: rc %d\n%s" % (fill, p.returncode, p.stderr[-1500:])
        row = json.loads(p.stdout.strip().splitlines()[-1])
        assert row["fill"] == fill
        out.append(row["rows"])
    assert len(out[0]) == len(references(17, 23)) and out[0] == out[1]
    assert [r[0] for r in out[0]] == [r["st"] for r in references(17, 23)]


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "helpers":
        os.environ["BSLV_LP_REV"] = "1"          # (read at create; _engine sets it too)
        _child_helpers()
    elif len(sys.argv) == 2 and sys.argv[1] == "fill":
        _child_fill()
