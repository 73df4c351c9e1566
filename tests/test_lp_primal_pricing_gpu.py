"""GPU: primal Devex pricing of the LP engine's primal steps (bslv_lpq_set_primal_pricing, include/bslv_hip.h) against the CPU yardsticks
of tests/lp_cases.py, the certificates (bslv_lpq_certify on the device, lp_cases.certify on the host) and the default rule.

  1  the update of the reference norms, exactly, on a crafted model of one primal pivot, in both forms
  2  objective batches ("cols", generations 1 and 2) at the shapes where the launch code changes its mind, in both forms
  3  the rule is not a no-op; the default rule counts nothing and has no norms to read
  4  an LP of at most one primal selection is the default rule's, bit for bit
  5  cold starts under PRIMAL, the mixed batch under REPAIR, and the precedence of the dual rule where both are on
  6  a periodic refactorisation starts new frameworks
  7  a detour through the switch leaves no trace; bad rules; the environment switch
  8  poisoned allocations
  9  end to end through BSLV_LP_PRIMAL_PRICING=devex: the dual Benson variant on ex01, ex05 and a covering problem

Run as a program (`python tests/test_lp_primal_pricing_gpu.py child`) it solves the (32, 65) "cols" set with the switch on and prints a
SHA-256 of everything it read: the fill-byte test starts it that way."""
import hashlib
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

from bensolve_amd.lp import LpEngine
import lp_cases as lc
from lp_cases import RTOL, OPTIMAL, UNDEFINED, NLP
from test_lp_general_gpu import _env, _engine, _read, _same_bits
from test_lp_obj_general_gpu import _feasible_start, _assert_against_references

pytestmark = pytest.mark.gpu

DANTZIG, DEVEX = 0, 1
E_ARG, E_STATE = 2, 5
TAB_SHAPES = [(16, 17), (32, 65), (33, 257), (24, 1536), (24, 2049)]
REV_SHAPES = [(33, 257), (24, 513), (24, 4100)]
CASES = [(M, N, "tableau") for M, N in TAB_SHAPES] + [(M, N, "revised") for M, N in REV_SHAPES]
NONE = np.zeros((1, 0))
GEN1, GEN2 = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(2))
POOL = 1 + 2 * NLP
ZERO = dict(weighted=0, other_col=0, resets=0)


def _batch(eng, src, dst, first, C, retry):
    """one objective batch: its record, the device certificate's verdicts, the counters and (under the rule) the norms of the batch
    itself; then, retry (the revised form), an LP that came back UNDEFINED once more from the feasibility solution in its slot, as
    test_lp_obj_general_gpu._solve_obj does"""
    st, it = eng.solve_batch_obj(src, dst, first, C)
    st, it = st.copy(), it.copy()
    stats = eng.last_primal_pricing_stats()
    norms = np.array([eng.last_primal_pricing_norms(b) for b in range(len(dst))]) if eng.get_primal_pricing() == DEVEX else None
    retries = 0
    if retry:
        for b in np.nonzero(st == UNDEFINED)[0]:
            _feasible_start(eng, dst[b], NONE, NONE)
            s1, i1 = eng.solve_batch_obj([dst[b]], [dst[b]], first, C[b:b + 1])
            st[b], it[b], retries = s1[0], it[b] + i1[0], retries + 1
    rec = _read(eng, dst, st, it)
    rec.update(stats=stats, norms=norms, retries=retries, verdict=eng.certify(dst, cost_first=first, costs=C)["verdict"])
    return rec


_RUNS = {}


def _single_costs(s, M, N):
    """NLP cost vectors with one entry each, +3 or -3 on a boxed column: short solves -- none, or one bound switch or pivot and
    whatever that leaves to do -- of which the objective sets' own generations have none"""
    lo, up = s["lo"][M:], s["up"][M:]
    boxed = np.nonzero(np.isfinite(lo) & np.isfinite(up) & (lo < up))[0]
    assert len(boxed) > 0
    C = np.zeros((NLP, N))
    for b in range(NLP):
        C[b, boxed[(b // 2) % len(boxed)]] = 3.0 if b % 2 == 0 else -3.0
    return C


def _run(M, N, form, rule, period=0):
    """generations 1 and 2 of the "cols" objective set of a shape in one form under one rule, once: the tests read the record"""
    key = (M, N, form, rule, period)
    if key not in _RUNS:
        s = lc.objective_set(M, N, "cols")
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL, form)
        assert eng.rows_folded() == 0
        assert eng.set_primal_pricing(rule) == 0 and eng.get_primal_pricing() == rule
        if period:
            assert eng.set_refactor_period(period) == 0
        _feasible_start(eng, 0, NONE, NONE)
        rec = dict(gen1=_batch(eng, np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"]["gen1"], form == "revised"))
        rec["gen2"] = _batch(eng, GEN1, GEN2, s["cost_first"], s["costs"]["gen2"], form == "revised")
        if form == "tableau":          # (after gen2 has read the slots of gen1)
            rec["single"] = _batch(eng, np.zeros(NLP, np.int32), GEN1, s["cost_first"], _single_costs(s, M, N), False)
        rec["period"] = eng.last_period_stats() if period else None
        eng.close()
        _RUNS[key] = rec
    return _RUNS[key]


def _check_against_yardsticks(M, N, form, rec):
    s = lc.objective_set(M, N, "cols")
    ref, oracle, _ = lc.assert_objective_references_agree(M, N, "cols")
    for g in ("gen1", "gen2"):
        got, tag = rec[g], (form, M, N, g)
        print("%s: pivots %s retries %d %s" % (tag, got["it"], got["retries"], got["stats"]))
        certs = _assert_against_references(s, s["folded"][g], ref[g], oracle["gap"], got, tag)      # statuses, both objectives at RTOL, the host certificate
        assert len(certs) == NLP, tag
        assert np.all(got["verdict"][got["st"] == OPTIMAL] == 0), (tag, got["verdict"])          # the device certificate
        t = got["norms"]
        assert t.shape == (NLP, M + N) and np.all(np.isfinite(t)) and np.all(t[t != 0.0] >= 1.0), tag
        assert np.all((t != 0.0).sum(axis=1) == N), tag          # (N nonbasic variables, M basic ones)


# ---- 1. the update, exactly ---------------------------------------------------------------------------------------------------
def crafted_model():
    """M = 2, N = 3, no singleton row, columns x >= 0, rows r_0 <= 1 and r_1 <= 6, zero own cost: the standard basis is feasible and the
    feasibility solve takes no pivot.  Under the costs (-1, 0.1, 0.1) column 0 enters, rows 0 and 1 block at 1 / 0.5 = 2 and 6 / 1 = 6:
    row 0 leaves on a pivot element of modulus 0.5 and the LP is optimal; under (1, 1, 1) nothing is eligible."""
    A = np.array([[0.5, 2.0, 1.0], [1.0, 3.0, 1.0]])
    M, N = A.shape
    lo = np.concatenate([np.full(M, -np.inf), np.zeros(N)])
    up = np.concatenate([[1.0, 6.0], np.full(N, np.inf)])
    return A, lo, up, np.zeros(N + 1), np.array([[-1.0, 0.1, 0.1], [1.0, 1.0, 1.0]])


def _crafted_run(form, rule):
    A, lo, up, cost, C = crafted_model()
    M, N = A.shape
    eng = _engine(A, lo, up, cost, 0, 0, 4, form)
    assert eng.rows_folded() == 0
    assert eng.set_primal_pricing(rule) == 0
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], NONE, NONE)
    assert st[0] == OPTIMAL and it[0] == 0, (st, it)
    st, it = eng.solve_batch_obj([0, 0], [1, 2], M, C)
    rec = _read(eng, [1, 2], st, it)
    rec["stats"] = eng.last_primal_pricing_stats()
    buf = np.zeros(M + N)
    if rule == DEVEX:
        rec["norms"] = [eng.last_primal_pricing_norms(0), eng.last_primal_pricing_norms(1)]
        assert eng.lib.bslv_lpq_last_primal_pricing_norms(eng.h, 2, buf.ctypes.data) == E_ARG          # (a batch of two)
        assert eng.lib.bslv_lpq_last_primal_pricing_norms(eng.h, -1, buf.ctypes.data) == E_ARG
    else:
        assert eng.lib.bslv_lpq_last_primal_pricing_norms(eng.h, 0, buf.ctypes.data) == E_STATE
    eng.close()
    return rec


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_the_update_exactly(form):
    A, lo, up, cost, C = crafted_model()
    M, N = A.shape
    rec = _crafted_run(form, DEVEX)
    assert list(rec["st"]) == [OPTIMAL, OPTIMAL] and list(rec["it"]) == [1, 0], (rec["st"], rec["it"])
    x, rows = rec["prim"][0][M:], rec["prim"][0][:M]
    moved = np.nonzero(x != 0.0)[0]
    assert len(moved) == 1, x
    q = int(moved[0])
    on_bound = np.nonzero(rows == up[:M])[0]
    assert len(on_bound) == 1, rows
    r = int(on_bound[0])
    assert (r, q) == (0, 0) and x[q] == 2.0
    exp = np.zeros(M + N)
    exp[M:] = np.maximum(1.0, np.abs(A[r] / A[r, q]))          # t_j = max(1, |alpha_rj / alpha_rq| * 1)
    exp[M + q] = 0.0                                            # the entering variable is basic
    exp[r] = max(1.0 / abs(A[r, q]), 1.0)                       # the leaving variable, nonbasic at position q
    t0, t1 = rec["norms"]
    print("norms after the pivot %s expected %s; LP without a pivot %s; %s" % (t0, exp, t1, rec["stats"]))
    assert np.array_equal(exp, [2.0, 0.0, 0.0, 4.0, 2.0])
    np.testing.assert_allclose(t0, exp, rtol=1e-15, atol=0.0)      # (the engine forms alpha_rj (1 / alpha_rq): two roundings against numpy's one)
    assert _same_bits(t1, np.array([0.0, 0.0, 1.0, 1.0, 1.0]))
    assert rec["stats"] == dict(weighted=1, other_col=0, resets=0)
    # the LP without a pivot is the default rule's bit for bit, and the other has the default rule's first (and only) selection
    off = _crafted_run(form, DANTZIG)
    assert off["stats"] == ZERO
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(rec[k], off[k]), (form, k)


# ---- 2. objective batches against the yardsticks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,form", CASES)
def test_objective_batches_under_primal_devex(oracle, M, N, form):
    _check_against_yardsticks(M, N, form, _run(M, N, form, DEVEX))


# ---- 3. not a no-op, and the default counts nothing -----------------------------------------------------------------------------------
def test_the_rule_changes_selections_and_the_default_counts_nothing(oracle):
    tot = dict(ZERO)
    for M, N in TAB_SHAPES:
        got = _run(M, N, "tableau", DEVEX)["gen1"]
        for k in tot:
            tot[k] += got["stats"][k]
    print("gen1 of %s under primal Devex: %s" % (TAB_SHAPES, tot))
    assert tot["other_col"] > 0 and tot["weighted"] >= tot["other_col"], tot
    for M, N in TAB_SHAPES:
        off = _run(M, N, "tableau", DANTZIG)
        for g in ("gen1", "gen2"):
            assert off[g]["stats"] == ZERO and off[g]["norms"] is None, (M, N, g, off[g]["stats"])
    s = lc.objective_set(32, 65, "cols")
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL, "tableau")
    _feasible_start(eng, 0, NONE, NONE)
    st, _ = eng.solve_batch_obj(np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"]["gen1"])
    buf = np.zeros(32 + 65)
    assert eng.lib.bslv_lpq_last_primal_pricing_norms(eng.h, 0, buf.ctypes.data) == E_STATE
    with pytest.raises(Exception):
        eng.last_primal_pricing_norms(0)
    eng.close()


# ---- 4. identity where it must hold -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", TAB_SHAPES)
def test_lps_of_at_most_one_selection_are_the_default_rules_bit_for_bit(oracle, M, N):
    """All norms are 1 until the first primal pivot of a solve has been made: an LP that the default rule solves in at most one
    iteration gets the same selection, and the same bits, under DEVEX (both from slot 0, which no rule has touched: the feasibility
    solve makes dual steps only)"""
    found = ones = 0
    for g in ("gen1", "single"):          # (single: cost vectors of one entry, see _single_costs -- the LPs of gen1 all take more than one iteration at some shapes)
        a, b = _run(M, N, "tableau", DANTZIG)[g], _run(M, N, "tableau", DEVEX)[g]
        assert np.all(a["st"] == OPTIMAL), (M, N, g, a["st"])
        few = np.nonzero(a["it"] <= 1)[0]
        print("%s %s: %d of %d LPs take at most one iteration under the default rule; iterations default %s devex %s" % ((M, N), g, len(few), NLP, a["it"], b["it"]))
        found += len(few); ones += int(np.sum(a["it"] == 1))
        for k in ("st", "it", "obj", "prim", "dual"):
            assert _same_bits(a[k][few], b[k][few]), (M, N, g, k, few)
    if found == 0 or ones == 0:
        pytest.skip("no LP of (%d, %d) takes one iteration under the default rule (%d take none)" % (M, N, found))


# ---- 5. methods ---------------------------------------------------------------------------------------------------------------------
def _cold(r, method, primal_rule, dual_rule=DANTZIG):
    M, N = r["A"].shape
    eng = LpEngine(M, N, r["A"], r["lo"], r["up"], r["cost"], 0, 0, 2)
    assert eng.set_method(method) == 0 and eng.set_primal_pricing(primal_rule) == 0 and eng.set_pricing(dual_rule) == 0
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], NONE, NONE)
    out = dict(st=int(st[0]), it=int(it[0]), obj=float(eng.obj([0])[0]), prim=eng.primal([0], 0, M + N)[0], dual=eng.dual([0], 0, M + N)[0],
               stats=eng.last_stats(), pricing=eng.last_primal_pricing_stats(), dual_pricing=eng.last_pricing_stats())
    eng.close()
    return out


def _check_cold(M, N, dual_rule):
    import test_lp_primal_gpu as tp
    ref = tp.references(M, N)
    tot = dict(ZERO, phase1_lps=0, dual_weighted=0)
    for t, r in enumerate(ref):
        assert r["st"] == r["st_highs"], (t, r["st"], r["st_highs"])
        got = _cold(r, tp.PRIMAL, DEVEX, dual_rule)
        assert got["st"] == r["st"], (M, N, t, got["st"], r["st"])          # (the infeasible and the unbounded LP among them)
        for k in ZERO:
            tot[k] += got["pricing"][k]
        tot["phase1_lps"] += got["stats"]["phase1_lps"]
        tot["dual_weighted"] += got["dual_pricing"]["weighted"] + got["dual_pricing"]["resets"]
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(got["obj"], r["obj"], rtol=1e-9, atol=1e-9, err_msg="lp %d" % t)
            np.testing.assert_allclose(got["obj"], r["obj_highs"], rtol=1e-9, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
            lc.check_optimality_conditions(r["A"], r["lo"], r["up"], r["cost"], got["obj"], got["prim"], got["dual"], (M, N, t))
    print("cold starts of (%d, %d) under PRIMAL, primal rule DEVEX, dual rule %d: %s" % (M, N, dual_rule, tot))
    return tot


@pytest.mark.parametrize("M,N", [(17, 23), (40, 70)])
def test_cold_start_under_primal_with_the_switch_on(oracle, M, N):
    tot = _check_cold(M, N, DANTZIG)
    assert tot["phase1_lps"] > 0 and tot["weighted"] > 0, tot
    assert tot["weighted"] >= tot["other_col"]


def test_both_rules_on_keep_the_dual_instance(oracle):
    """a PRIMAL batch with both rules on runs the dual-Devex instance: the references' answers, and the primal counters read 0"""
    tot = _check_cold(17, 23, DEVEX)
    assert tot["phase1_lps"] > 0 and tot["dual_weighted"] > 0, tot
    assert {k: tot[k] for k in ZERO} == ZERO, tot


def test_mixed_batch_under_repair_equals_its_lps_alone_with_the_switch_on():
    import test_lp_primal_gpu as tp
    with _env(BSLV_LP_PRIMAL_PRICING="devex"):          # (read at create: the engine of that test is created with the rule)
        eng, M, N, lo, up = tp._row_range_engine(303, 2)
        assert eng.get_primal_pricing() == DEVEX
        eng.close()
        tp.test_mixed_batch_under_repair_equals_its_lps_alone()


# ---- 6. new frameworks --------------------------------------------------------------------------------------------------------------
def test_periodic_refactorisation_starts_new_frameworks(oracle):
    M, N = 33, 257
    rec = _run(M, N, "revised", DEVEX, period=6)
    _check_against_yardsticks(M, N, "revised", rec)
    resets = rec["gen1"]["stats"]["resets"] + rec["gen2"]["stats"]["resets"]
    print("period 6: %s, resets %d" % (rec["period"], resets))
    assert resets > 0


# ---- 7. the default is untouched -----------------------------------------------------------------------------------------------------
def test_a_detour_through_the_switch_leaves_no_trace(oracle):
    M, N = 32, 65
    s = lc.objective_set(M, N, "cols")
    fresh = _run(M, N, "tableau", DANTZIG)["gen1"]
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL + 1, "tableau")
    _feasible_start(eng, 0, NONE, NONE)
    assert eng.get_primal_pricing() == DANTZIG
    assert eng.set_primal_pricing(DEVEX) == 0
    st, _ = eng.solve_batch_obj([0], [POOL], s["cost_first"], s["costs"]["gen2"][:1])          # one objective solve in a spare slot
    assert st[0] == OPTIMAL and eng.last_primal_pricing_stats()["weighted"] > 0
    assert eng.set_primal_pricing(2) == E_ARG and eng.set_primal_pricing(-1) == E_ARG and eng.get_primal_pricing() == DEVEX
    assert eng.set_primal_pricing(DANTZIG) == 0
    assert eng.set_primal_pricing(2) == E_ARG and eng.get_primal_pricing() == DANTZIG
    got = _batch(eng, np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"]["gen1"], False)
    eng.close()
    assert got["stats"] == ZERO
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(got[k], fresh[k]), k
    with _env(BSLV_LP_PRIMAL_PRICING="devex"):
        e2 = LpEngine(M, N, s["A"], s["lo"], s["up"], s["cost"], 0, 0, 2)
    assert e2.get_primal_pricing() == DEVEX and e2.get_pricing() == DANTZIG
    e2.close()
    with _env(BSLV_LP_PRIMAL_PRICING="dantzig"):
        e3 = LpEngine(M, N, s["A"], s["lo"], s["up"], s["cost"], 0, 0, 2)
    assert e3.get_primal_pricing() == DANTZIG
    e3.close()


# ---- 8. poisoned allocations ---------------------------------------------------------------------------------------------------------
def _child():
    rec = _run(32, 65, "tableau", DEVEX)
    h = hashlib.sha256()
    for g in ("gen1", "gen2"):
        for k in ("st", "it", "obj", "prim", "dual", "norms", "verdict"):
            h.update(np.ascontiguousarray(rec[g][k]).tobytes())
        h.update(repr(sorted(rec[g]["stats"].items())).encode())
    print("fill %s statuses %s" % (os.environ.get("BSLV_FILL"), "".join(str(v) for g in ("gen1", "gen2") for v in rec[g]["st"])))
    print("sha256 " + h.hexdigest())


def test_the_rule_does_not_depend_on_the_fill_byte():
    """BSLV_FILL (read once per process) is the byte fresh device allocations are filled with: nothing the rule reads -- the norms
    among it -- may be memory that nobody wrote.  One fresh child process per fill byte."""
    out = []
    for fill in ("0x00", "0x7F"):
        env = dict(os.environ, BSLV_FILL=fill)
        for k in ("BSLV_LP_REV", "BSLV_ALLOC_LOG", "BSLV_LP_PRIMAL_PRICING", "BSLV_LP_PRICING"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
        assert "Memory access fault" not in p.stderr, "fill %s: %s" % (fill, p.stderr[-800:])
        assert p.returncode == 0, "fill %s: rc %d\n%s" % (fill, p.returncode, p.stderr[-1500:])      # (the first child that fails ends the test)
        lines = p.stdout.strip().splitlines()
        print(lines[-2])
        assert lines[-2].split()[:2] == ["fill", fill] and lines[-2].split()[3] == str(OPTIMAL) * (2 * NLP), lines[-2]
        out.append(lines[-1])
    assert out[0].startswith("sha256 ") and out[0] == out[1], out


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex", ["ex01", "ex05"])
def test_cli_dual_variant_under_the_environment_switch_matches_the_goldens(tmp_path, ex):
    from test_cli_gpu import CLI, EXDIR, EX_TOL, GOLD, _gold_rows, read_img      # (the comparison of test_cli_all_phases_match_hybrid_goldens)
    base = os.path.join(tmp_path, ex)
    r = subprocess.run([CLI, os.path.join(EXDIR, ex + ".vlp"), "-m", "2", "-B", "64", "-a", "dual", "-o", base],
                       env=dict(os.environ, BSLV_LP_PRIMAL_PRICING="devex"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for side in ("p", "d"):
        t, X, _ = read_img(base + "_img_%s.sol" % side)
        gt, gX = _gold_rows(GOLD["%s/%s_type" % (ex, side)], GOLD["%s/%s" % (ex, side)])
        assert np.array_equal(t, gt), (ex, side, r.stdout)
        np.testing.assert_allclose(X, gX, rtol=EX_TOL, atol=EX_TOL)


def test_covering_problem_through_the_dual_variant_against_the_default_rule():
    """covering_vlp(40, 20, 4, 9) through the dual Benson variant under both rules: other pivots may end on another optimal point of a
    degenerate P1(w), hence other cuts -- both results must approximate the same pair of images within eps: every vertex of either
    upper image satisfies every cut (vertex of the lower image) of the other, and of its own (the comparison of
    tests/test_lp_pricing_gpu.py, test_covering_problem_to_termination_against_the_default_rule)"""
    from bensolve_amd import synth
    from bensolve_amd.vlp import solve_primal
    prob = synth.covering_vlp(40, 20, 4, 9)
    eps = 1e-7
    res = {}
    for name, rule in (("default", None), ("devex", "devex")):
        with _env(BSLV_LP_PRIMAL_PRICING=rule):
            out = solve_primal(prob, bounded=True, batch=32, eps_benson_phase2=eps, alg_phase2="dual")
        assert out["status"] == "optimal", out["message"]
        d = out["dump"]
        X = d["X"][d["pu"].astype(bool) & (d["pi"] == 0)]
        Y = d["Y"][d["du"].astype(bool) & (d["di"] == 0)]
        res[name] = (X, Y, out["lps"])
    names = list(res)
    scale = max(1.0, max(np.abs(res[n][0]).max() for n in names))
    for a in names:
        for b in names:
            X, Y = res[a][0], res[b][1]
            w = np.hstack([Y[:, :-1], 1 - Y[:, :-1].sum(axis=1, keepdims=True)])
            worst = float((X @ w.T - Y[:, -1][None, :]).min())
            assert worst >= -5 * eps * scale, "vertices of '%s' violate a cut of '%s' by %.3e (eps %.0e)" % (a, b, -min(worst, 0.0), eps)
    print("primal pricing rules, dual variant: " + ", ".join("%s: %d vertices, %d facets, %d LPs" % (n, len(res[n][0]), len(res[n][1]), res[n][2]) for n in names))
    assert len(res["default"][0]) > 100


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "child":
        _child()
