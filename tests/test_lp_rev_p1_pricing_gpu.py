"""GPU: Devex pricing for PRIMAL / REPAIR batches of the REVISED LP form, per call (bslv_lpq_solve_batch_method_priced:
k_select_priced_p1_rev<RULE_PDV> and <RULE_DVX> in bensolve_amd/csrc/lp_engine.hip), against the CPU yardsticks the project already has
-- the oracle's primal simplex (oracle/lp_dense.c) and HiGHS, check_optimality_conditions, the device certificate -- and never against
the engine itself, except where an identity is the claim.  Optimal values: lp_cases.RTOL = 1e-9 relative, atol 1e-9; statuses equal.

The LP sets are those of tests/test_lp_rev_primal_gpu.py (seeds chosen on the CPU so that both yardsticks agree on every LP): the
sets of test_lp_primal_gpu.lp_set at (6, 5), (17, 23), (40, 70) and lp_cases.general_set at the revised form's launch thresholds
(33, 257), (24, 1536), (24, 2049), (24, 4100).  Every test first asserts that the yardsticks agree, then looks at the engine.

The two rule pairs (dual rule, primal rule): "pdv" = (DANTZIG, DEVEX), the primal-Devex instance; "dvx" = (DEVEX, DANTZIG), the
dual-Devex instance.  No shape needed a refactorisation period to keep the pivot cross-check quiet.

Run as a program: `python tests/test_lp_rev_p1_pricing_gpu.py helpers` runs the (24, 4100) cold batch of arrangement "a" under both
rule pairs and prints a SHA-256 per pair; `... fill` solves the (17, 23) cold-start set under primal Devex and prints statuses and
objective bits as one JSON line."""
import ctypes
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
import oracle_api
from lp_cases import RTOL, NLP, check_optimality_conditions
from test_lp_general_gpu import _engine, _env, _same_bits
from test_lp_primal_gpu import lp_set, references, _row_range_engine
import test_lp_rev_primal_gpu as rp
from test_lp_rev_primal_gpu import _read, _assert_bits, _counters, _digest, _row_range_engine_rev, _mixed_bounds, _dual_batch_bounds

pytestmark = pytest.mark.gpu

DUAL, PRIMAL, REPAIR = 0, 1, 2
OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED = 4, 0, 1, 3
DANTZIG, DEVEX = 0, 1
E_ARG = 2
NONE = np.zeros((1, 0))
SMALL = rp.SMALL
EDGES = rp.EDGES
RULES = dict(pdv=(DANTZIG, DEVEX), dvx=(DEVEX, DANTZIG))
ZERO_P = dict(weighted=0, other_col=0, resets=0)
ZERO_D = dict(weighted=0, other_row=0, resets=0)


def _pricing(eng):
    return dict(primal=eng.last_primal_pricing_stats(), dual=eng.last_pricing_stats())


def _norms(eng, B):
    """both norm read-outs of the last call, None where the call ran no instance of the rule"""
    out = []
    for f in (eng.last_pricing_norms, eng.last_primal_pricing_norms):
        try:
            out.append(np.array([f(b) for b in range(B)]))
        except Exception:
            out.append(None)
    return out


def _same_norms(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and _same_bits(x, y)) for x, y in zip(a, b))


# ---- the small sets, one LP per engine, cold and in place ---------------------------------------------------------------------------------
_SMALL = {}


def cold_set_priced(M, N, rule, method=PRIMAL):
    """every LP of test_lp_primal_gpu.lp_set(M, N) from a reset slot of a revised engine under `method` and the rule pair, once"""
    key = (M, N, rule, method)
    if key not in _SMALL:
        dr, pr = rule
        rows = []
        for A, lo, up, cost in lp_set(M, N):
            eng = _engine(A, lo, up, cost, 0, 0, 2, "revised")
            eng.reset_slot(0)
            st, it = eng.solve_batch_method_priced(method, dr, pr, [0], [0], NONE, NONE)
            rows.append(dict(st=int(st[0]), iters=int(it[0]), obj=float(eng.obj([0])[0]), prim=eng.primal([0], 0, M + N)[0], dual=eng.dual([0], 0, M + N)[0],
                             stats=eng.last_stats(), pricing=_pricing(eng)))
            eng.close()
        _SMALL[key] = rows
    return _SMALL[key]


def _check_small(M, N, rule):
    """the references' statuses and objectives and the optimality conditions of every LP; returns the counters summed over the shape"""
    ref = references(M, N)
    assert ref[0]["st"] == INFEASIBLE and ref[1]["st"] == UNBOUNDED                 # the two built on purpose
    for t, r in enumerate(ref):
        assert r["st"] == r["st_highs"], (t, r["st"], r["st_highs"])                # (the yardsticks agree)
    tot = dict(phase1_lps=0, iters=0, primal=dict(ZERO_P), dual=dict(ZERO_D))
    for t, (r, got) in enumerate(zip(ref, cold_set_priced(M, N, rule))):
        assert got["st"] == r["st"], (M, N, rule, t, got["st"], r["st"])
        tot["phase1_lps"] += got["stats"]["phase1_lps"]
        tot["iters"] += got["iters"]
        for side in ("primal", "dual"):
            for k, v in got["pricing"][side].items():
                tot[side][k] += v
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(got["obj"], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
            np.testing.assert_allclose(got["obj"], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
            check_optimality_conditions(r["A"], r["lo"], r["up"], r["cost"], got["obj"], got["prim"], got["dual"], (M, N, t))
    print("cold starts of (%d, %d), revised form, PRIMAL, rules %s: %s" % (M, N, rule, tot))
    return tot


# ---- 1. cold starts against the yardsticks, small shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SMALL)
def test_cold_start_under_primal_devex_small_shapes(oracle, M, N):
    tot = _check_small(M, N, RULES["pdv"])
    assert tot["phase1_lps"] > 0 and tot["primal"]["weighted"] > 0, tot
    assert tot["primal"]["weighted"] >= tot["primal"]["other_col"] and tot["dual"] == ZERO_D, tot


@pytest.mark.parametrize("M,N", SMALL)
def test_cold_start_under_dual_devex_small_shapes(oracle, M, N):
    """the dual-Devex instance under PRIMAL: its own triple counts the dual selections it weighted ([0]) and the frameworks its primal
    and phase-1 pivots started ([2]); the primal triple reads 0.  A cold PRIMAL solve of these sets makes no dual selection at all --
    measured: weighted 0 at all three shapes, resets 108 / 1124 / 4872 -- so what shows that the instance ran is weighted + resets, as
    in test_lp_primal_pricing_gpu.test_both_rules_on_keep_the_dual_instance; the dual rule's weighted > 0 is asserted where dual
    selections exist, in the mixed batch under REPAIR below"""
    tot = _check_small(M, N, RULES["dvx"])
    assert tot["phase1_lps"] > 0 and tot["dual"]["weighted"] + tot["dual"]["resets"] > 0, tot
    assert tot["primal"] == ZERO_P, tot


# ---- 2. cold batches at the launch thresholds: 16 LPs, one lock-step batch from 16 reset slots in place ---------------------------------
_COLD = {}


def cold_batch_priced(M, N, arr, rule, method=PRIMAL, period=0, rescue=False):
    key = (M, N, arr, rule, method, period, rescue)
    if key not in _COLD:
        dr, pr = rule
        s = lc.general_set(M, N, arr)
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], NLP, "revised")
        if period:
            assert eng.set_refactor_period(period) == 0
        if rescue:
            assert eng.set_refactor(1) == 0
        dst = np.arange(NLP, dtype=np.int32)
        for k in dst:
            eng.reset_slot(int(k))
        st, it = eng.solve_batch_method_priced(method, dr, pr, dst, dst, s["vlo"], s["vup"])
        rec = _read(eng, dst, st, it)
        rec.update(stats=eng.last_stats(), pricing=_pricing(eng), period=eng.last_period_stats(), rfx=eng.last_refactor_stats(),
                   getters=(eng.get_pricing(), eng.get_primal_pricing(), eng.get_method()))
        rec["verdict"] = eng.certify(dst, s["vlo"], s["vup"])["verdict"]
        eng.close()
        _COLD[key] = rec
    return _COLD[key]


def _check_batch(M, N, arr, rec, tag):
    ref, _ = lc.assert_references_agree(M, N, arr)          # (LP BAD INFEASIBLE, at least 12 OPTIMAL, both yardsticks agree)
    print("%s (%d, %d) %s: statuses %s pivots %s %s %s" % (tag, M, N, arr, rec["st"], rec["it"], _counters(rec["stats"]), rec["pricing"]))
    assert not np.any(rec["st"] == UNDEFINED), rec["st"]
    assert np.array_equal(rec["st"], [r["st"] for r in ref]), (rec["st"], [r["st"] for r in ref])
    for t, r in enumerate(ref):
        if r["st"] != OPTIMAL:
            continue
        np.testing.assert_allclose(rec["obj"][t], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
        np.testing.assert_allclose(rec["obj"][t], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
        assert rec["verdict"][t] == 0, (t, rec["verdict"])
    return ref


@pytest.mark.parametrize("rule", ["pdv", "dvx"])
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", EDGES)
def test_cold_batch_at_the_launch_thresholds(oracle, M, N, arr, rule):
    rec = cold_batch_priced(M, N, arr, RULES[rule])
    _check_batch(M, N, arr, rec, "cold PRIMAL batch under " + rule)
    assert rec["stats"]["phase1_lps"] == NLP and rec["stats"]["phase1_iterations"] > 0, rec["stats"]
    assert rec["pricing"]["dual" if rule == "pdv" else "primal"] == (ZERO_D if rule == "pdv" else ZERO_P), rec["pricing"]


def test_the_rules_are_not_no_ops_at_the_launch_thresholds(oracle):
    other_col = dvx = 0
    for M, N in EDGES:
        lc.assert_references_agree(M, N, "a")
        other_col += cold_batch_priced(M, N, "a", RULES["pdv"])["pricing"]["primal"]["other_col"]
        d = cold_batch_priced(M, N, "a", RULES["dvx"])["pricing"]["dual"]
        dvx += d["weighted"] + d["resets"]
    print("summed over %s: other_col under primal Devex %d, weighted + resets under dual Devex %d" % (EDGES, other_col, dvx))
    assert other_col > 0 and dvx > 0


# ---- 3. the norm update, exactly -----------------------------------------------------------------------------------------------------------
def _one_pivot(A, lo, up, cost):
    """(engine record, the oracle's pivot count) of one cold PRIMAL solve under primal Devex in the revised form"""
    M, N = A.shape
    olp = oracle_api.OracleLP(A, lo, up, cost)
    ost, opiv = olp.solve(0), olp.pivots()
    ox = olp.primal(0, M + N)
    olp.close()
    assert ost == OPTIMAL and opiv == 1, (ost, opiv)          # (the CPU first: exactly that one pivot)
    eng = _engine(A, lo, up, cost, 0, 0, 2, "revised")
    assert eng.rows_folded() == 0
    eng.reset_slot(0)
    st, it = eng.solve_batch_method_priced(PRIMAL, DANTZIG, DEVEX, [0], [0], NONE, NONE)
    rec = dict(st=int(st[0]), it=int(it[0]), prim=eng.primal([0], 0, M + N)[0], norms=eng.last_primal_pricing_norms(0), stats=eng.last_stats(), pricing=_pricing(eng), ox=ox)
    eng.close()
    return rec


def _expected_norms(A, r, q):
    M, N = A.shape
    exp = np.zeros(M + N)
    exp[M:] = np.maximum(1.0, np.abs(A[r] / A[r, q]))          # t_j = max(1, |alpha_rj / alpha_rq| * 1)
    exp[M + q] = 0.0                                            # the entering variable is basic
    exp[r] = max(1.0 / abs(A[r, q]), 1.0)                       # the leaving variable, nonbasic at position q
    return exp


def test_the_update_exactly_after_a_phase2_pivot(oracle):
    """test_lp_primal_pricing_gpu.crafted_model with its first cost vector as the engine's own cost: the standard basis is primal feasible
    and dual infeasible, column 0 enters, row 0 leaves on a pivot element of 0.5, and the LP is optimal"""
    A = np.array([[0.5, 2.0, 1.0], [1.0, 3.0, 1.0]])
    M, N = A.shape
    lo = np.concatenate([np.full(M, -np.inf), np.zeros(N)])
    up = np.concatenate([[1.0, 6.0], np.full(N, np.inf)])
    rec = _one_pivot(A, lo, up, np.array([0.0, -1.0, 0.1, 0.1]))
    assert (rec["st"], rec["it"]) == (OPTIMAL, 1) and rec["stats"]["phase1_lps"] == 0, rec
    assert rec["prim"][M + 0] == 2.0 and rec["prim"][0] == up[0] and np.array_equal(rec["prim"], rec["ox"]), rec["prim"]      # (r, q) = (0, 0)
    exp = _expected_norms(A, 0, 0)
    print("norms after the phase-2 pivot %s expected %s %s" % (rec["norms"], exp, rec["pricing"]))
    assert np.array_equal(exp, [2.0, 0.0, 0.0, 4.0, 2.0])
    np.testing.assert_allclose(rec["norms"], exp, rtol=1e-15, atol=0.0)
    assert rec["pricing"]["primal"] == dict(weighted=1, other_col=0, resets=0) and rec["pricing"]["dual"] == ZERO_D


def test_the_update_exactly_after_a_phase1_pivot(oracle):
    """zero cost, row 0 >= 1 with the coefficients (0.5, -2, -1), row 1 <= 6, columns >= 0: the standard basis is infeasible in row 0, only
    column 0 lowers the infeasibility, row 0 blocks at its bound on a pivot element of 0.5 -- one PHASE-1 pivot (0, 0), after which the LP
    is feasible and, having no cost, optimal.  The norms are not all 1: |alpha_0j / alpha_00| = (., 4, 2), 1 / |alpha_00| = 2"""
    A = np.array([[0.5, -2.0, -1.0], [1.0, 3.0, 1.0]])
    M, N = A.shape
    lo = np.concatenate([[1.0, -np.inf], np.zeros(N)])
    up = np.concatenate([[np.inf, 6.0], np.full(N, np.inf)])
    rec = _one_pivot(A, lo, up, np.zeros(N + 1))
    assert (rec["st"], rec["it"]) == (OPTIMAL, 1), rec
    assert rec["stats"]["phase1_lps"] == 1 and rec["stats"]["phase1_iterations"] == 1, rec["stats"]
    assert rec["prim"][M + 0] == 2.0 and rec["prim"][0] == lo[0] and np.array_equal(rec["prim"], rec["ox"]), rec["prim"]      # (r, q) = (0, 0)
    exp = _expected_norms(A, 0, 0)
    print("norms after the phase-1 pivot %s expected %s %s" % (rec["norms"], exp, rec["pricing"]))
    assert not np.all(exp[exp != 0.0] == 1.0)
    np.testing.assert_allclose(rec["norms"], exp, rtol=1e-15, atol=0.0)
    assert rec["pricing"]["primal"] == dict(weighted=1, other_col=0, resets=0) and rec["pricing"]["dual"] == ZERO_D


# ---- 4. identities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(17, 23), (33, 257)])
def test_lps_of_at_most_one_selection_are_the_default_rules_bit_for_bit(oracle, M, N):
    """all norms are 1 until the first pivot of a solve has been made: an LP that solve_batch_method(PRIMAL) solves in at most one
    selection gets the same selection, and the same bits, under either rule"""
    if (M, N) == (17, 23):
        for r in references(M, N):
            assert r["st"] == r["st_highs"]
        plain = rp.cold_set_rev(M, N)
        few = [t for t, g in enumerate(plain) if g["iters"] <= 1]
        for rule in RULES.values():
            got = cold_set_priced(M, N, rule)
            for t in few:
                assert plain[t]["st"] == got[t]["st"] and plain[t]["iters"] == got[t]["iters"], (rule, t)
                for k in ("obj", "prim", "dual"):
                    assert _same_bits(np.asarray(plain[t][k]), np.asarray(got[t][k])), (rule, t, k)
    else:
        lc.assert_references_agree(M, N, "a")
        plain = rp.cold_batch(M, N, "a")
        few = np.nonzero(plain["it"] <= 1)[0]
        for rule in RULES.values():
            got = cold_batch_priced(M, N, "a", rule)
            for k in rp.KEYS:
                assert _same_bits(plain[k][few], got[k][few]), (rule, k, few)
    print("(%d, %d): LPs of at most one selection under the default rule: %s" % (M, N, list(few)))
    if len(few) == 0:
        pytest.skip("no LP of the (%d, %d) cold set takes at most one selection under the default rule" % (M, N))


def test_both_rules_dantzig_is_solve_batch_method(oracle):
    M, N, arr = 24, 2049, "a"
    lc.assert_references_agree(M, N, arr)
    a, b = rp.cold_batch(M, N, arr), cold_batch_priced(M, N, arr, (DANTZIG, DANTZIG))
    _assert_bits(a, b, "both rules DANTZIG against solve_batch_method")
    assert _counters(a["stats"]) == _counters(b["stats"]), (a["stats"], b["stats"])
    assert b["pricing"] == dict(primal=ZERO_P, dual=ZERO_D), b["pricing"]
    assert np.array_equal(a["verdict"], b["verdict"])


@pytest.mark.parametrize("rule", ["pdv", "dvx"])
@pytest.mark.parametrize("method", [DUAL, PRIMAL, REPAIR])
def test_tableau_form_the_call_is_the_switch_sequence(method, rule):
    """two twin engines of the tableau form at (17, 23), the mixed batch of test_lp_rev_primal_gpu: the call against set_pricing;
    set_primal_pricing; solve_batch_method; <both old switches back> -- records, counters, both stats triples and both norm read-outs"""
    B = 16
    dr, pr = RULES[rule]
    out = []
    for by_call in (True, False):
        eng, M, N, lo, up = _row_range_engine(303, B + 1)
        vlo, vup = _mixed_bounds(eng, M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        src = np.zeros(B, np.int32)
        if by_call:
            st, it = eng.solve_batch_method_priced(method, dr, pr, src, dst, vlo, vup)
        else:
            assert eng.set_pricing(dr) == 0 and eng.set_primal_pricing(pr) == 0
            st, it = eng.solve_batch_method(method, src, dst, vlo, vup)
            assert eng.set_pricing(DANTZIG) == 0 and eng.set_primal_pricing(DANTZIG) == 0
        assert (eng.get_pricing(), eng.get_primal_pricing(), eng.get_method()) == (DANTZIG, DANTZIG, DUAL)
        rec = _read(eng, dst, st, it)
        rec.update(stats=_counters(eng.last_stats()), pricing=_pricing(eng), norms=_norms(eng, B))
        out.append(rec)
        eng.close()
    print("method %d rules %s: statuses %s %s" % (method, rule, out[0]["st"], out[0]["pricing"]))
    _assert_bits(out[0], out[1], ("the call against the switch sequence", method, rule))
    assert out[0]["stats"] == out[1]["stats"] and out[0]["pricing"] == out[1]["pricing"], (out[0]["stats"], out[1]["stats"], out[0]["pricing"], out[1]["pricing"])
    assert _same_norms(out[0]["norms"], out[1]["norms"])
    assert (out[0]["norms"][0] is not None) == (rule == "dvx") and (out[0]["norms"][1] is not None) == (rule == "pdv" and method != DUAL)


@pytest.mark.parametrize("rule", ["pdv", "dvx"])
def test_revised_form_dual_is_set_pricing_and_solve_batch(rule):
    B = 12
    dr, pr = RULES[rule]
    out = []
    for by_call in (True, False):
        eng, M, N, lo, up = _row_range_engine_rev(303, B + 1)
        vlo, vup = _dual_batch_bounds(M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        src = np.zeros(B, np.int32)
        if by_call:
            st, it = eng.solve_batch_method_priced(DUAL, dr, pr, src, dst, vlo, vup)
        else:
            assert eng.set_pricing(dr) == 0
            st, it = eng.solve_batch(src, dst, vlo, vup)
            assert eng.set_pricing(DANTZIG) == 0
        assert np.all(st == OPTIMAL), st
        assert (eng.get_pricing(), eng.get_primal_pricing(), eng.get_method()) == (DANTZIG, DANTZIG, DUAL)
        rec = _read(eng, dst, st, it)
        rec.update(stats=_counters(eng.last_stats()), pricing=_pricing(eng), norms=_norms(eng, B))
        out.append(rec)
        eng.close()
    _assert_bits(out[0], out[1], ("DUAL through the call against set_pricing + solve_batch", rule))
    assert out[0]["stats"] == out[1]["stats"] and out[0]["pricing"] == out[1]["pricing"], (out[0]["pricing"], out[1]["pricing"])
    assert _same_norms(out[0]["norms"], out[1]["norms"])
    assert out[0]["pricing"]["primal"] == ZERO_P and out[0]["norms"][1] is None          # (the primal rule does not reach a DUAL batch)
    assert (out[0]["norms"][0] is not None) == (rule == "dvx")


def test_both_rules_devex_keep_the_dual_instance(oracle):
    tot = _check_small(17, 23, (DEVEX, DEVEX))
    assert tot["phase1_lps"] > 0 and tot["dual"]["weighted"] + tot["dual"]["resets"] > 0, tot
    assert tot["primal"] == ZERO_P, tot


# ---- 5. batch against alone, and helpers ---------------------------------------------------------------------------------------------------
def test_cold_batch_equals_its_lps_alone(oracle):
    M, N, arr = 24, 2049, "a"
    lc.assert_references_agree(M, N, arr)
    dr, pr = RULES["pdv"]
    together = cold_batch_priced(M, N, arr, (dr, pr))
    s = lc.general_set(M, N, arr)
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], NLP, "revised")
    st, it = [], []
    for b in range(NLP):
        eng.reset_slot(b)
        s1, i1 = eng.solve_batch_method_priced(PRIMAL, dr, pr, [b], [b], s["vlo"][b:b + 1], s["vup"][b:b + 1])
        st.append(s1[0]); it.append(i1[0])
    alone = _read(eng, np.arange(NLP, dtype=np.int32), st, it)
    eng.close()
    _assert_bits(together, alone, "16 together against 16 alone under primal Devex")


@pytest.mark.parametrize("rule", ["pdv", "dvx"])
def test_mixed_batch_under_repair_equals_its_lps_alone(rule):
    B = 16
    dr, pr = RULES[rule]
    eng, M, N, lo, up = _row_range_engine_rev(303, 2 * B + 1)
    vlo, vup = _mixed_bounds(eng, M, lo, up, B)
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch_method_priced(REPAIR, dr, pr, np.zeros(B, np.int32), dst, vlo, vup)
    stats, pricing = eng.last_stats(), _pricing(eng)
    print("batch under %s: statuses %s iters %s %s %s" % (rule, st, it, _counters(stats), pricing))
    assert 0 < stats["phase1_lps"] < B, stats       # some need phase 1, some none
    assert np.all(st != UNDEFINED), st
    assert pricing["primal" if rule == "pdv" else "dual"]["weighted"] > 0, pricing
    together = _read(eng, dst, st, it)
    alone = dict(st=[], it=[])
    dst1 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    for b in range(B):
        s1, i1 = eng.solve_batch_method_priced(REPAIR, dr, pr, [0], [dst1[b]], vlo[b:b + 1], vup[b:b + 1])
        alone["st"].append(s1[0]); alone["it"].append(i1[0])
    _assert_bits(together, _read(eng, dst1, alone["st"], alone["it"]), ("batch against single LPs", rule))
    eng.close()


def _child_helpers():
    for rule in ("pdv", "dvx"):
        rec = cold_batch_priced(24, 4100, "a", RULES[rule])
        print("%s helpers %s statuses %s sha256 %s" % (rule, os.environ.get("BSLV_REV_HELPERS"), "".join(str(v) for v in rec["st"]), _digest(rec)))


def test_cold_batch_does_not_depend_on_the_number_of_helpers(oracle):
    ref, _ = lc.assert_references_agree(24, 4100, "a")
    want = "".join(str(r["st"]) for r in ref)
    out = []
    for helpers in ("1", None):
        env = dict(os.environ)
        env.pop("BSLV_REV_HELPERS", None)
        if helpers:
            env["BSLV_REV_HELPERS"] = helpers
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "helpers"], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, "helpers %s: rc %d\n%s" % (helpers, p.returncode, p.stderr[-1500:])      # (the first child that fails ends the test)
        lines = p.stdout.strip().splitlines()[-2:]
        print("\n".join(lines))
        assert [l.split()[0] for l in lines] == ["pdv", "dvx"] and all(l.split()[4] == want for l in lines), lines
        out.append([l.split()[-1] for l in lines])
    assert out[0] == out[1] and all(len(v) == 64 for v in out[0]), out


# ---- 6. refactorisation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["pdv", "dvx"])
def test_periodic_refactorisation_starts_new_frameworks(oracle, rule):
    M, N, K = 33, 257, 6
    rec = cold_batch_priced(M, N, "a", RULES[rule], period=K)
    _check_batch(M, N, "a", rec, "period %d under %s" % (K, rule))
    print("period %d: %s, phase 1 %s" % (K, rec["period"], {k: v for k, v in rec["stats"].items() if k.startswith("phase1")}))
    assert rec["pricing"]["primal" if rule == "pdv" else "dual"]["resets"] > 0, rec["pricing"]
    # refactorisations in the rounds, and LPs still in phase 1 when they were due: more phase-1 iterations than K for each of the NLP LPs
    # together means one LP at least spent more than K of them there
    assert rec["period"]["in_rounds"] > 0 and rec["stats"]["phase1_iterations"] > K * NLP, (rec["period"], rec["stats"])


@pytest.mark.parametrize("rule", ["pdv", "dvx"])
def test_the_rescue_resolves_under_the_calls_method_and_rule(oracle, rule):
    """set_refactor(1) and the hook BSLV_LP_REV_DRIFT=0:3 (the cross-check of LP 0 counts as failed at its third pivot): LP 0 is marked,
    its inverse rebuilt and the LP solved again inside the call.  The basis it had reached is primal infeasible (a cold start, two
    pivots in), so only a re-solve under PRIMAL ends in the references' answer; the re-solve's counters are added to the call's"""
    M, N = 33, 257
    with _env(BSLV_LP_REV_DRIFT="0:3"):
        rec = cold_batch_priced(M, N, "a", RULES[rule], rescue=True)
    ref = _check_batch(M, N, "a", rec, "rescue under %s" % rule)
    print("rescue: %s" % rec["rfx"])
    assert ref[0]["st"] == OPTIMAL and rec["rfx"]["rescued"] == 1 and rec["rfx"]["failed"] == 0, rec["rfx"]
    plain = cold_batch_priced(M, N, "a", RULES[rule])
    assert rec["stats"]["phase1_lps"] == plain["stats"]["phase1_lps"] + 1, (rec["stats"], plain["stats"])      # (LP 0 entered phase 1 twice)
    side = "primal" if rule == "pdv" else "dual"
    assert rec["pricing"][side]["weighted"] + rec["pricing"][side]["resets"] > 0 and rec["pricing"]["dual" if rule == "pdv" else "primal"] in (ZERO_D, ZERO_P), rec["pricing"]
    assert rec["getters"] == (DANTZIG, DANTZIG, DUAL)


# ---- 7. no trace ---------------------------------------------------------------------------------------------------------------------------
def test_a_priced_call_leaves_no_trace():
    B = 12
    out = []
    for detour in (False, True):
        eng, M, N, lo, up = _row_range_engine_rev(303, 2 * B + 2)
        assert eng.set_pricing(DEVEX) == 0 and eng.set_primal_pricing(DEVEX) == 0      # (switches that do not reach the batch below, and must come back as they are)
        vlo, vup = _dual_batch_bounds(M, lo, up, B)
        dst = np.arange(1, B + 1, dtype=np.int32)
        src = np.zeros(B, np.int32)
        if detour:
            st, _ = eng.solve_batch_method_priced(PRIMAL, DANTZIG, DEVEX, [0], [2 * B + 1], lo[None, :M], up[None, :M])       # a solve in another slot
            assert st[0] == OPTIMAL
            assert (eng.get_pricing(), eng.get_primal_pricing(), eng.get_method()) == (DEVEX, DEVEX, DUAL)
            # refused arguments change nothing
            st7, it7 = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
            f = eng.lib.bslv_lpq_solve_batch_method_priced
            f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
            for method, dr, pr in ((7, 0, 0), (-1, 0, 1), (PRIMAL, 2, 0), (PRIMAL, 0, -1), (PRIMAL, -1, -1)):
                assert f(eng.h, method, dr, pr, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data, st7.ctypes.data, it7.ctypes.data) == E_ARG, (method, dr, pr)
            assert f(None, PRIMAL, 0, 1, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data, st7.ctypes.data, it7.ctypes.data) == E_ARG
            assert np.all(st7 == -7) and np.all(it7 == -7)
            assert (eng.get_pricing(), eng.get_primal_pricing(), eng.get_method()) == (DEVEX, DEVEX, DUAL)
        st, it = eng.solve_batch_method(PRIMAL, src, dst, vlo, vup)
        assert np.all(st == OPTIMAL), st
        rec = _read(eng, dst, st, it)
        rec.update(stats=_counters(eng.last_stats()), pricing=_pricing(eng))
        out.append(rec)
        eng.close()
    _assert_bits(out[0], out[1], "fresh engine against one after a priced call")
    assert out[0]["stats"] == out[1]["stats"], (out[0]["stats"], out[1]["stats"])
    assert out[0]["pricing"] == out[1]["pricing"] == dict(primal=ZERO_P, dual=ZERO_D)


# ---- 8. poisoned allocations ---------------------------------------------------------------------------------------------------------------
def _child_fill():
    rows = [[g["st"], g["obj"].hex() if g["st"] == OPTIMAL else None] for g in cold_set_priced(17, 23, RULES["pdv"])]
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
