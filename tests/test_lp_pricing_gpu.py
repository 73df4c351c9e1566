"""GPU: dual Devex pricing of the LP engine (bslv_lpq_set_pricing, the DVX instances of select_once in lp_engine.hip) against the two
CPU yardsticks of tests/lp_cases.py, the device certificate (bslv_lpq_certify) and the default rule.

Under DEVEX every basis row of an LP has a reference norm s_i >= 1, all 1 at the start of a solve; the violated row with the largest
violation / s_i leaves, and a dual pivot on row r with the multipliers f_i leaves s_i = max(s_i, |f_i| s_r), s_r = max(s_r / |pivot|, 1).
So: same statuses and optimal values as the default rule, other pivots -- and the SAME pivots wherever all norms are still 1.

  1  the general sets of tests/lp_cases.py at the shape edges of the launch code, both forms and the extended selection, in the run
     sequence of tests/test_lp_general_gpu.py (cold LP, batch of 16, alone, second generation, in place)
  2  tall shapes, where the row loops of Phases A and D take a second trip: (255, 24) and (257, 24) at 256 threads, (1025, 24) at 1024
  3  the update itself on a crafted LP of one pivot, in both forms
  4  the rule is not a no-op: over the cold starts of (33, 257) and (257, 24) some selection takes another row than the default
  5  identity where all norms are 1: LPs of at most one pivot, and the switch set and cleared again
  6  interplay: methods REPAIR and PRIMAL, canonical duals, periodic refactorisation, objective batches
  7  end to end through BSLV_LP_PRICING=devex: ex01's known answer, a covering problem against the default rule"""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bensolve_amd.lp import LpEngine, P2Model
import lp_cases as lc
from lp_cases import RTOL, OPTIMAL, INFEASIBLE, UNDEFINED, NLP, BAD

pytestmark = pytest.mark.gpu

DANTZIG, DEVEX = 0, 1
E_ARG, E_STATE = 2, 5
TAB_SHAPES = [(15, 16), (16, 17), (32, 65), (33, 257), (24, 1121), (24, 1536), (24, 2049)]
REV_SHAPES = [(33, 257), (24, 2049), (24, 4100)]
EXT_SHAPES = [(32, 65)]
CASES = [(M, N, "tableau") for M, N in TAB_SHAPES] + [(M, N, "revised") for M, N in REV_SHAPES] + [(M, N, "extended") for M, N in EXT_SHAPES]
NONE = np.zeros((1, 0))
# slots: 0 the parent; the batch; its LPs alone; the second generation; scratch
GEN1, ALONE, GEN2, SCRATCH = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(4))
POOL = 1 + 4 * NLP


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(A, lo, up, cost, first, cnt, slots, form, pricing):
    """form: "tableau", "revised" (BSLV_LP_REV=1, read at create) or "extended" (the tableau form with set_extended(1))"""
    M, N = A.shape
    with _env(BSLV_LP_REV="1" if form == "revised" else None, BSLV_LP_PRICING=None):
        eng = LpEngine(M, N, A, lo, up, cost, first, cnt, slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [__import__("ctypes").c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(form == "revised")
    if form == "extended":
        eng.set_extended(1)
    assert eng.get_pricing() == DANTZIG
    assert eng.set_pricing(pricing) == 0 and eng.get_pricing() == pricing
    return eng


def _solve(eng, src, dst, vlo, vup, retry):
    """one batch; retry (the revised form): an LP that comes back UNDEFINED is solved once more from a reset slot, as the header tells
    callers to.  Returns statuses, pivots, the number of retries and the pricing counters of the batch."""
    st, it = eng.solve_batch(src, dst, vlo, vup)
    ps = eng.last_pricing_stats()
    st, it, n = st.copy(), it.copy(), 0
    if retry:
        for b in np.nonzero(st == UNDEFINED)[0]:
            eng.reset_slot(int(dst[b]))
            s1, i1 = eng.solve_batch([dst[b]], [dst[b]], vlo[b:b + 1], vup[b:b + 1])
            st[b], it[b], n = s1[0], it[b] + i1[0], n + 1
    return st, it, n, ps


def _read(eng, dst, st, it, vlo, vup, ps=None):
    """what a batch left in its slots, with the verdicts of the device certificate at its default tolerances"""
    n = eng.M + eng.N
    dst = np.asarray(dst, np.int32)
    return dict(st=np.array(st), it=np.array(it), obj=eng.obj(dst), prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n),
                verdict=eng.certify(dst, vlo, vup)["verdict"], pricing=ps)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


_RUNS = {}


def _run(M, N, arr, form, pricing):
    """every solve of one set in one form under one rule, once: the tests only look at the record.  The sequence of
    tests/test_lp_general_gpu.py; under DEVEX, behind it, the batch of 16 from a parent that the DEFAULT rule solved, under both
    rules on this engine ("from_default_dantzig", "from_default_devex": the same start for the comparison bit for bit)."""
    key = (M, N, arr, form, pricing)
    if key in _RUNS:
        return _RUNS[key]
    s = lc.general_set(M, N, arr)
    vlo, vup, perm = s["vlo"], s["vup"], s["perm"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, form, pricing)
    rec = dict(retries=0)
    zeros = np.zeros(NLP, np.int32)

    def batch(name, src, dst, lo, up, count=True):
        st, it, n, ps = _solve(eng, src, dst, lo, up, retry and count)
        rec[name] = _read(eng, dst, st, it, lo, up, ps)
        if count:
            rec["retries"] += n

    eng.reset_slot(0)
    batch("cold", [0], [0], vlo[:1], vup[:1])
    if pricing == DEVEX:
        rec["cold_norms"] = eng.last_pricing_norms(0) if rec["retries"] == 0 else None
    batch("gen1", zeros, GEN1, vlo, vup)
    if form == "tableau":
        st, it = [], []
        for b in range(NLP):
            s1, i1 = eng.solve_batch([0], [ALONE[b]], vlo[b:b + 1], vup[b:b + 1])
            st.append(s1[0]); it.append(i1[0])
        rec["gen1_alone"] = _read(eng, ALONE, st, it, vlo, vup)
    if pricing == DANTZIG:
        eng.close()
        _RUNS[key] = rec
        return rec
    batch("gen2", GEN1, GEN2, vlo[perm], vup[perm])
    batch("again", GEN2, GEN2, vlo[perm], vup[perm], count=False)
    # the parent once more, by the default rule; then its children under both rules
    assert eng.set_pricing(DANTZIG) == 0
    eng.reset_slot(0)
    batch("cold_default", [0], [0], vlo[:1], vup[:1], count=False)
    batch("from_default_dantzig", zeros, SCRATCH, vlo, vup, count=False)
    assert eng.set_pricing(DEVEX) == 0
    batch("from_default_devex", zeros, ALONE, vlo, vup, count=False)
    eng.close()
    _RUNS[key] = rec
    return rec


def _assert_against_references(s, ref, oracle_gap, got, lps, tag):
    """statuses, objectives (both yardsticks), the device certificate and the CPU certificate of every OPTIMAL LP of one batch"""
    for b, t in enumerate(lps):
        r = ref[t]
        assert got["st"][b] == r["st"], (tag, b, t, got["st"], [ref[u]["st"] for u in lps])
        if r["st"] != OPTIMAL:
            continue
        np.testing.assert_allclose(got["obj"][b], r["obj"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d" % (tag, t))
        np.testing.assert_allclose(got["obj"][b], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d (HiGHS)" % (tag, t))
        assert got["verdict"][b] == 0, (tag, b, t, got["verdict"])
        lo, up = s["lps"][t]
        c = lc.certify(s["A"], lo, up, s["cost"], int(got["st"][b]), got["obj"][b], got["prim"][b], got["dual"][b])
        lc.assert_certified(c, got["obj"][b], oracle_gap, (tag, b, t))


# ---- 1. general sets at the shape edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N,form", CASES)
def test_devex_on_a_general_set(oracle, M, N, form, arr):
    s = lc.general_set(M, N, arr)
    ref, oracle_w = lc.assert_references_agree(M, N, arr)
    rec = _run(M, N, arr, form, DEVEX)
    perm = s["perm"]
    tag = (form, M, N, arr)
    print("pivots %s: cold %s gen1 %s gen2 %s retries %d pricing cold %s gen1 %s gen2 %s" % (
        tag, rec["cold"]["it"], rec["gen1"]["it"], rec["gen2"]["it"], rec["retries"], rec["cold"]["pricing"], rec["gen1"]["pricing"], rec["gen2"]["pricing"]))
    _assert_against_references(s, ref, oracle_w["gap"], rec["cold"], [0], tag + ("cold",))
    _assert_against_references(s, ref, oracle_w["gap"], rec["gen1"], range(NLP), tag + ("gen1",))
    _assert_against_references(s, ref, oracle_w["gap"], rec["gen2"], perm, tag + ("gen2",))
    assert rec["gen1"]["st"][BAD] == INFEASIBLE
    for gen in ("cold", "gen1", "gen2"):
        assert not np.any(rec[gen]["st"] == UNDEFINED), (tag, gen, rec[gen]["st"])
    if form != "revised":
        assert rec["retries"] == 0
    for gen in ("cold", "gen1", "gen2"):
        p = rec[gen]["pricing"]
        assert p["weighted"] >= p["other_row"] >= 0 and p["resets"] >= 0, (tag, gen, p)
    if form == "tableau":          # a batch is its LPs alone, bit for bit, under this rule too
        for k in ("st", "it", "obj", "prim", "dual"):
            assert _same_bits(rec["gen1"][k], rec["gen1_alone"][k]), (tag, k)
    # again in place: nothing to do for an LP that is solved
    again, gen2 = rec["again"], rec["gen2"]
    assert np.array_equal(again["st"], gen2["st"]), (tag, again["st"], gen2["st"])
    opt = gen2["st"] == OPTIMAL
    assert np.all(again["it"][opt] == 0), (tag, again["it"])
    if rec["cold_norms"] is not None:
        assert np.all(np.isfinite(rec["cold_norms"])) and np.all(rec["cold_norms"] >= 1.0)


# ---- 2. tall shapes ------------------------------------------------------------------------------------------------------
# (M, N) -> (seed, BSLV_SELECT_NT).  M = 255 / 257: the loop over the M rows of Phase A and the M + 1 entries of Phase D at 256 threads
# (one trip / one and a row / two); M = 1025 the same at 1024 threads.  The seeds were chosen on the CPU: HiGHS and the oracle agree
# on all 8 LPs of each set to 1e-13 (python tests/test_lp_pricing_gpu.py).
TALL = {(255, 24): (101, None), (257, 24): (102, None), (1025, 24): (103, "1024")}
TALL_NLP, TALL_CNT = 8, 12


_TALL = {}


def tall_set(M, N):
    """lc.random_lp's feasible and bounded LP and 8 LPs over a per-LP range of the first 12 columns: LP 0 has the model's bounds, LP t
    widens or narrows the finite sides of the range by whole numbers around the point the model was built on (it stays inside, the
    LP feasible; the finite and infinite sides stay what they are, the contract of a DUAL start)."""
    if (M, N) in _TALL:
        return _TALL[(M, N)]
    seed = TALL[(M, N)][0]
    rng = np.random.default_rng(seed)
    A, lo, up, cost, x0, tr, tc = lc.random_lp(M, N, rng, "feasible", bounded=True, parts=True)
    first, cnt = M, TALL_CNT
    vlo, vup = np.tile(lo[first:first + cnt], (TALL_NLP, 1)), np.tile(up[first:first + cnt], (TALL_NLP, 1))
    x = x0[:cnt]
    fixed = lo[first:first + cnt] == up[first:first + cnt]
    for t in range(1, TALL_NLP):
        l, u = x - rng.integers(0, 2 + t // 2, size=cnt), x + rng.integers(0, 2 + t // 2, size=cnt)
        u = np.where(~fixed & (u == l), l + 1, u)
        vlo[t] = np.where(fixed, vlo[0], np.where(np.isfinite(vlo[0]), l, vlo[0]))
        vup[t] = np.where(fixed, vup[0], np.where(np.isfinite(vup[0]), u, vup[0]))
    lps = []
    for t in range(TALL_NLP):
        l, u = lo.copy(), up.copy()
        l[first:first + cnt], u[first:first + cnt] = vlo[t], vup[t]
        lps.append((l, u))
    out = dict(M=M, N=N, A=A, lo=lo, up=up, cost=cost, var_first=first, var_cnt=cnt, vlo=vlo, vup=vup, lps=lps)
    _TALL[(M, N)] = out
    return out


_TALL_REF = {}


def tall_references(M, N):
    """both yardsticks on the 8 LPs of a tall set, asserted to agree; rows of dict(st, obj, obj_highs), and the oracle's worst gap"""
    if (M, N) not in _TALL_REF:
        s = tall_set(M, N)
        rows = []
        for lo, up in s["lps"]:
            so, zo, po, do = lc.oracle_solution(s["A"], lo, up, s["cost"])
            sh, zh = lc.highs(s["A"], lo, up, s["cost"])
            assert so == sh == OPTIMAL, (M, N, so, sh)
            np.testing.assert_allclose(zo, zh, rtol=RTOL, atol=1e-9)
            rows.append(dict(st=so, obj=zo, st_highs=sh, obj_highs=zh, cert=lc.certify(s["A"], lo, up, s["cost"], so, zo, po, do)))
        _TALL_REF[(M, N)] = (rows, lc.worst([r["cert"] for r in rows]))
    return _TALL_REF[(M, N)]


_TALL_RUNS = {}


def _tall_run(M, N, pricing):
    if (M, N, pricing) in _TALL_RUNS:
        return _TALL_RUNS[(M, N, pricing)]
    s = tall_set(M, N)
    with _env(BSLV_SELECT_NT=TALL[(M, N)][1]):
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], TALL_NLP + 1, "tableau", pricing)
        assert eng.rows_folded() == 0
        rec = {}
        eng.reset_slot(0)
        st, it, _, ps = _solve(eng, [0], [0], s["vlo"][:1], s["vup"][:1], False)
        rec["cold"] = _read(eng, [0], st, it, s["vlo"][:1], s["vup"][:1], ps)
        rec["cold_norms"] = eng.last_pricing_norms(0)[None] if pricing == DEVEX else None
        dst = np.arange(1, TALL_NLP + 1, dtype=np.int32)
        st, it, _, ps = _solve(eng, np.zeros(TALL_NLP, np.int32), dst, s["vlo"], s["vup"], False)
        rec["gen1"] = _read(eng, dst, st, it, s["vlo"], s["vup"], ps)
        rec["gen1_norms"] = np.array([eng.last_pricing_norms(b) for b in range(TALL_NLP)]) if pricing == DEVEX else None
        eng.close()
    _TALL_RUNS[(M, N, pricing)] = rec
    return rec


@pytest.mark.parametrize("M,N", sorted(TALL))
def test_devex_on_a_tall_set(oracle, M, N):
    s = tall_set(M, N)
    ref, w = tall_references(M, N)
    rec = _tall_run(M, N, DEVEX)
    tag = ("tall", M, N)
    print("pivots %s: cold %s gen1 %s pricing cold %s gen1 %s largest norm %.3g" % (tag, rec["cold"]["it"], rec["gen1"]["it"], rec["cold"]["pricing"], rec["gen1"]["pricing"],
                                                                                 max(rec["cold_norms"].max(), rec["gen1_norms"].max())))
    _assert_against_references(s, ref, w["gap"], rec["cold"], [0], tag + ("cold",))
    _assert_against_references(s, ref, w["gap"], rec["gen1"], range(TALL_NLP), tag + ("gen1",))
    for norms in (rec["cold_norms"], rec["gen1_norms"]):
        assert norms.shape[1] == M
        assert np.all(np.isfinite(norms)) and np.all(norms >= 1.0)
    assert rec["cold"]["it"][0] > 1 and rec["cold_norms"].max() > 1.0          # (the cold start pivots: some norm has moved)


# ---- 3. the update, exactly -------------------------------------------------------------------------------------------------
def crafted_model():
    """M = 5, N = 4, no singleton row.  Columns x >= 0 with costs (1, 4, 4, 4): the standard basis is dual feasible.  Row 0 is per LP:
    r_0 >= 1 is violated at x = 0 and the ratio test takes column 0 (1 / 0.5 against 4 / 1); after the pivot x_0 = 2 and the rows
    1 .. 4, in [-10, 10], hold 6, -2, 0.5 and 8: feasible, one pivot."""
    A = np.array([[0.5, 1.0, 1.0, 1.0],
                  [3.0, 1.0, 0.0, 2.0],
                  [-1.0, 0.0, 1.0, 1.0],
                  [0.25, 2.0, 1.0, 0.0],
                  [4.0, 1.0, 1.0, 0.0]])
    M, N = A.shape
    lo = np.concatenate([[-np.inf], np.full(M - 1, -10.0), np.zeros(N)])
    up = np.concatenate([[np.inf], np.full(M - 1, 10.0), np.full(N, np.inf)])
    lo[0] = -1.0
    cost = np.array([0.0, 1.0, 4.0, 4.0, 4.0])
    return A, lo, up, cost


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_the_update_exactly(form):
    A, lo, up, cost = crafted_model()
    M, N = A.shape
    eng = _engine(A, lo, up, cost, 0, 1, 4, form, DEVEX)
    assert eng.rows_folded() == 0
    vlo, vup = np.array([[1.0], [-1.0]]), np.array([[np.inf], [np.inf]])          # LP 0: row 0 >= 1 (one pivot); LP 1: row 0 >= -1 (none)
    eng.reset_slot(0)
    st, it = eng.solve_batch([0, 0], [1, 2], vlo, vup)
    assert list(st) == [OPTIMAL, OPTIMAL] and list(it) == [1, 0], (st, it)
    x = eng.primal([1], M, N)[0]
    s0, s1 = eng.last_pricing_norms(0), eng.last_pricing_norms(1)
    stats = eng.last_pricing_stats()
    buf = np.zeros(M)
    assert eng.lib.bslv_lpq_last_pricing_norms(eng.h, 2, buf.ctypes.data) == E_ARG          # (a batch of two)
    eng.close()
    r = 0                                       # the one row violated at the standard basis
    moved = np.nonzero(x != lo[M:])[0]
    assert len(moved) == 1, x
    q = int(moved[0])
    assert q == 0 and x[q] == 2.0
    exp = np.maximum(1.0, np.abs(A[:, q] / A[r, q]))
    exp[r] = max(1.0 / abs(A[r, q]), 1.0)
    print("norms after the pivot %s expected %s; LP without a pivot %s; %s" % (s0, exp, s1, stats))
    assert np.array_equal(exp, [2.0, 6.0, 2.0, 1.0, 8.0])
    np.testing.assert_allclose(s0, exp, rtol=1e-15, atol=0.0)       # (the engine forms a_iq (1 / a_rq): two roundings against numpy's one)
    assert np.array_equal(s1, np.ones(M))
    assert stats == dict(weighted=1, other_row=0, resets=0)


# ---- 4. the rule is not a no-op -------------------------------------------------------------------------------------------
def test_the_rule_changes_selections_and_the_default_counts_nothing(oracle):
    tot = dict(weighted=0, other_row=0, resets=0)
    rows = [_run(33, 257, arr, "tableau", DEVEX)["cold"] for arr in ("a", "b")] + [_tall_run(257, 24, DEVEX)["cold"]]
    for got in rows:
        assert got["st"][0] == OPTIMAL
        for k in tot:
            tot[k] += got["pricing"][k]
    print("cold starts of (33, 257) a / b and (257, 24) under Devex: %s; pivots %s" % (tot, [int(g["it"][0]) for g in rows]))
    assert tot["other_row"] > 0 and tot["weighted"] >= tot["other_row"], tot
    off = [_run(33, 257, arr, "tableau", DANTZIG)["cold"] for arr in ("a", "b")] + [_tall_run(257, 24, DANTZIG)["cold"]]
    print("... under the default rule: pivots %s" % [int(g["it"][0]) for g in off])
    for got in off:
        assert got["pricing"] == dict(weighted=0, other_row=0, resets=0), got["pricing"]


def test_norms_are_refused_while_the_switch_is_off():
    A, lo, up, cost = crafted_model()
    eng = _engine(A, lo, up, cost, 0, 1, 4, "tableau", DANTZIG)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [1], np.array([[1.0]]), np.array([[np.inf]]))
    assert st[0] == OPTIMAL
    buf = np.zeros(A.shape[0])
    assert eng.lib.bslv_lpq_last_pricing_norms(eng.h, 0, buf.ctypes.data) == E_STATE
    assert eng.set_pricing(2) == E_ARG and eng.set_pricing(-1) == E_ARG and eng.get_pricing() == DANTZIG
    with _env(BSLV_LP_PRICING="devex"):
        e2 = LpEngine(A.shape[0], A.shape[1], A, lo, up, cost, 0, 1, 4)
    assert e2.get_pricing() == DEVEX
    e2.close()
    eng.close()


# ---- 5. identity where it must hold ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N,form", CASES)
def test_lps_of_at_most_one_pivot_are_the_default_rules_bit_for_bit(oracle, M, N, form, arr):
    """All norms are 1 until the first pivot of a solve has been made: an LP that the default rule solves in at most one pivot gets the
    same pivot, and the same bits, under DEVEX -- from the same start: the parent of the batches compared was solved by the default
    rule.  And an engine whose switch was on and is off again is a fresh engine."""
    dvx, fresh = _run(M, N, arr, form, DEVEX), _run(M, N, arr, form, DANTZIG)
    a, b = dvx["from_default_dantzig"], dvx["from_default_devex"]
    few = np.nonzero(a["it"] <= 1)[0]
    print("%s: %d of %d LPs of the batch take at most one pivot under the default rule; pivots default %s devex %s" % ((form, M, N, arr), len(few), NLP, a["it"], b["it"]))
    assert len(few) > 0
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(a[k][few], b[k][few]), (form, M, N, arr, k, few)
    if fresh["cold"]["it"][0] <= 1 and dvx["retries"] == 0 and fresh["retries"] == 0:
        for k in ("st", "it", "obj", "prim", "dual"):
            assert _same_bits(dvx["cold"][k], fresh["cold"][k]), (form, M, N, arr, "cold", k)
    # back to DANTZIG on the engine that ran under DEVEX: a fresh engine's cold LP and batch
    if form != "revised" or (fresh["retries"] == 0 and not np.any(a["st"] == UNDEFINED)):
        for name, other in (("cold_default", "cold"), ("from_default_dantzig", "gen1")):
            for k in ("st", "it", "obj", "prim", "dual"):
                assert _same_bits(dvx[name][k], fresh[other][k]), (form, M, N, arr, name, k)
            assert dvx[name]["pricing"] == dict(weighted=0, other_row=0, resets=0)


# ---- 6. interplay ---------------------------------------------------------------------------------------------------------
def test_methods_repair_and_primal_under_devex(oracle):
    """a warm start that is dual infeasible (a nonbasic row loses the bound it sits on) and primal infeasible (a basic row gets an
    upper bound below its value), as in tests/test_lp_primal_gpu.py, on the (32, 65) set: phase 1, primal steps, then dual steps
    under the weighted rule.  Every phase-1 or primal pivot starts a new reference framework."""
    M, N = 32, 65
    s = lc.general_set(M, N, "a")                 # every row is per LP
    A, cost, lo, up = s["A"], s["cost"], s["lo"], s["up"]
    eng = _engine(A, lo, up, cost, s["var_first"], s["var_cnt"], 8, "tableau", DANTZIG)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], s["vlo"][:1], s["vup"][:1])
    assert st[0] == OPTIMAL
    prim, dual = eng.primal([0], 0, M + N)[0], eng.dual([0], 0, M + N)[0]
    nonbasic = [k for k in range(M) if abs(dual[k]) > 1e-3]
    basic = [k for k in range(M) if dual[k] == 0.0 and prim[k] - lo[k] > 1.0 and up[k] - prim[k] > 1e-6]
    assert nonbasic and basic
    chosen = None
    for kn in nonbasic:
        for kb in basic:
            lo2, up2 = lo.copy(), up.copy()
            if dual[kn] > 0: lo2[kn] = -np.inf
            else: up2[kn] = np.inf
            up2[kb] = prim[kb] - 0.5
            so, zo, po, do = lc.oracle_solution(A, lo2, up2, cost)
            sh, zh = lc.highs(A, lo2, up2, cost)
            if so == OPTIMAL and sh == OPTIMAL:
                chosen = (lo2, up2, zo, zh, lc.certify(A, lo2, up2, cost, so, zo, po, do)["gap"])
                break
        if chosen:
            break
    assert chosen, "no pair of changes leaves a solvable LP"
    lo2, up2, zo, zh, ogap = chosen
    vlo, vup = lo2[None, :M].copy(), up2[None, :M].copy()
    st, _ = eng.solve_batch([0], [1], vlo, vup)
    assert st[0] == UNDEFINED                       # the default method cannot start there
    assert eng.set_pricing(DEVEX) == 0
    for method, dst in ((2, 2), (1, 3)):
        assert eng.set_method(method) == 0
        st, it = eng.solve_batch([0], [dst], vlo, vup)
        ps, ls = eng.last_pricing_stats(), eng.last_stats()
        got = _read(eng, [dst], st, it, vlo, vup)
        print("method %d under Devex: status %d pivots %d obj %r (oracle %r) pricing %s phase 1 LPs %d primal steps %d" % (method, st[0], it[0], got["obj"][0], zo, ps, ls["phase1_lps"], ls["primal_steps"]))
        assert st[0] == OPTIMAL, (method, st)
        np.testing.assert_allclose(got["obj"][0], zo, rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(got["obj"][0], zh, rtol=RTOL, atol=1e-9)
        assert ls["phase1_lps"] == 1 and ps["resets"] >= 1, (ps, ls)
        assert got["verdict"][0] == 0, got["verdict"]
        c = lc.certify(A, lo2, up2, cost, OPTIMAL, got["obj"][0], got["prim"][0], got["dual"][0])
        lc.assert_certified(c, got["obj"][0], ogap, ("method", method))
        norms = eng.last_pricing_norms(0)
        assert np.all(np.isfinite(norms)) and np.all(norms >= 1.0)
    eng.close()


def test_canonical_duals_under_devex():
    """the tie phase never reads the norms, and the canonical basis does not depend on the pivots that led to the optimum: the duals
    are the ones tests/test_lp_canonical_gpu.py expects, at its tolerance"""
    import canonical_cases as cc
    prob, c = cc.cases("octahedron")
    cc.check_case_set(c)
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    with _env(BSLV_LP_PRICING=None):
        eng = LpEngine.from_model(model, pool_slots=B + 2)
    assert eng.set_pricing(DEVEX) == 0
    ub = model.ub_for(V)
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), ub[:1])
    assert st0[0] == OPTIMAL
    assert eng.set_canonical(1, cc.direction(model.q) @ model.R) == 0
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.full((B, model.r), -np.inf), ub)
    w, z = eng.dual(dst, model.w_first, model.q), eng.obj(dst)
    ps, cs = eng.last_pricing_stats(), eng.last_canonical_stats()
    eng.close()
    print("octahedron under Devex: pricing %s tie phase %s largest |w - expected| %.3e" % (ps, cs, np.abs(w - c["w"]).max()))
    assert np.all(st == OPTIMAL)
    np.testing.assert_allclose(z, c["z"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(w, c["w"], rtol=1e-9, atol=1e-9)
    assert ps["weighted"] > 0


def test_periodic_refactorisation_under_devex(oracle):
    """revised form, (24, 2049), an LP's inverse rebuilt once it is 12 steps old: every replay during the rounds starts a new reference
    framework (counted), the answers stay the yardsticks'"""
    M, N, arr = 24, 2049, "a"
    s = lc.general_set(M, N, arr)
    ref, w = lc.assert_references_agree(M, N, arr)
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, "revised", DEVEX)
    assert eng.set_refactor_period(12) == 0
    replays = resets = primal = 0
    eng.reset_slot(0)
    st, it, n, ps = _solve(eng, [0], [0], s["vlo"][:1], s["vup"][:1], False)
    per, ls = eng.last_period_stats(), eng.last_stats()
    replays += per["in_rounds"]; resets += ps["resets"]; primal += ls["primal_steps"]
    cold = _read(eng, [0], st, it, s["vlo"][:1], s["vup"][:1])
    print("cold: status %s pivots %s period %s pricing %s" % (st, it, per, ps))
    st, it, n, ps = _solve(eng, np.zeros(NLP, np.int32), GEN1, s["vlo"], s["vup"], False)
    per, ls = eng.last_period_stats(), eng.last_stats()
    replays += per["in_rounds"]; resets += ps["resets"]; primal += ls["primal_steps"]
    gen1 = _read(eng, GEN1, st, it, s["vlo"], s["vup"])
    print("gen1: status %s pivots %s period %s pricing %s" % (st, it, per, ps))
    norms = eng.last_pricing_norms(NLP - 1)
    eng.close()
    _assert_against_references(s, ref, w["gap"], cold, [0], ("period", "cold"))
    _assert_against_references(s, ref, w["gap"], gen1, range(NLP), ("period", "gen1"))
    assert replays > 0, "no LP grew 12 steps old: the test does not reach the replay"
    assert resets == replays + primal, (resets, replays, primal)
    assert np.all(np.isfinite(norms)) and np.all(norms >= 1.0)


def test_objective_batches_do_not_see_the_switch():
    """solve_batch_obj makes primal steps only: with the switch on it runs the kernels it always ran, and no bit differs.  (From the
    same start: the feasible basis in the parent's slot comes from a dual solve, which the rule does change -- the default rule's in
    both engines.)"""
    M, N = 32, 65
    s = lc.objective_set(M, N, "cols")
    out = []
    for pricing in (DANTZIG, DEVEX):
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, NLP + 1, "tableau", DANTZIG)
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [0], NONE, NONE)
        assert st[0] == OPTIMAL
        assert eng.set_pricing(pricing) == 0 and eng.get_pricing() == pricing
        st, it = eng.solve_batch_obj(np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"]["gen1"])
        ps = eng.last_pricing_stats()
        n = M + N
        out.append(dict(st=st.copy(), it=it.copy(), obj=eng.obj(GEN1), prim=eng.primal(GEN1, 0, n), dual=eng.dual(GEN1, 0, n)))
        assert ps == dict(weighted=0, other_row=0, resets=0), ps
        eng.close()
    assert np.all(out[0]["st"] == OPTIMAL) and out[0]["it"].sum() > 0
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(out[0][k], out[1][k]), k


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def test_ex01_known_answer_under_the_environment_switch():
    """ex/example01.m: the upper image has the vertices (0, 4) and (-6, 6) and the extreme directions (1, 0) and (-1, 1)"""
    from bensolve_amd import synth
    from bensolve_amd.vlp import solve_primal
    prob = synth.read_vlp(os.path.join(ROOT, "tests", "golden", "ex", "ex01.vlp"))
    with _env(BSLV_LP_PRICING="devex"):
        out = solve_primal(prob, batch=8)
    assert out["status"] == "optimal", out
    d = out["dump"]
    live = d["pu"].astype(bool)
    pts = d["X"][live & ~d["pi"].astype(bool)]
    dirs = d["X"][live & d["pi"].astype(bool)]
    dirs = dirs / np.abs(dirs).max(axis=1, keepdims=True)
    assert sorted(map(tuple, np.round(pts, 9) + 0.0)) == [(-6.0, 6.0), (0.0, 4.0)]
    assert sorted(map(tuple, np.round(dirs, 9) + 0.0)) == [(-1.0, 1.0), (1.0, 0.0)]


def test_covering_problem_to_termination_against_the_default_rule():
    """covering_vlp(40, 20, 4, 9) to termination under both rules: other pivots may end on other optimal bases of a degenerate P2(v),
    hence other cuts -- both results must be outer approximations of the same upper image within eps: every vertex of either satisfies
    every cut of the other (the comparison of tests/test_benson_gpu.py,
    test_families_and_newest_first_give_outer_approximations_of_the_same_image)"""
    from bensolve_amd import synth
    from bensolve_amd.benson import BensonEngine
    prob = synth.covering_vlp(40, 20, 4, 9)
    eps, batch = 1e-7, 128
    res = {}
    for name, rule in (("default", None), ("devex", "devex")):
        with _env(BSLV_LP_PRICING=rule):
            eng = BensonEngine(prob, eps=eps, pool_slots=4 * batch + 64)
            assert eng.start() == 0
            eng.run(batch)
            d = eng.poly_dump()
            tot = eng.totals()
            eng.close()
        assert np.all(d["ps"][d["pu"].astype(bool)] == 1)
        X = d["X"][d["pu"].astype(bool) & (d["pi"] == 0)]
        Y = d["Y"][d["du"].astype(bool) & (d["di"] == 0)]
        res[name] = (X, Y, tot)
    names = list(res)
    scale = max(1.0, max(np.abs(res[n][0]).max() for n in names))
    for a, b in ((names[0], names[1]), (names[1], names[0])):
        X, Y = res[a][0], res[b][1]
        w = np.hstack([Y[:, :-1], 1 - Y[:, :-1].sum(axis=1, keepdims=True)])
        worst = float((X @ w.T - Y[:, -1][None, :]).min())
        assert worst >= -5 * eps * scale, "vertices of '%s' violate a cut of '%s' by %.3e (eps %.0e)" % (a, b, -min(worst, 0.0), eps)
    print("pricing rules: " + ", ".join("%s: %d vertices, %d facets, %d LPs" % (n, len(res[n][0]), len(res[n][1]), res[n][2]["lps"]) for n in names))
    assert len(res["default"][0]) > 100


if __name__ == "__main__":
    # the check made on the CPU when the seeds of the tall sets were chosen: both yardsticks on every LP
    import time
    for (M, N) in sorted(TALL):
        t0 = time.time()
        rows, w = tall_references(M, N)
        print("tall set M %d N %d seed %d: statuses %s largest |oracle - HiGHS| %.3e oracle gap %.3e (%.1f s)" % (
            M, N, TALL[(M, N)][0], "".join(str(r["st"]) for r in rows), max(abs(r["obj"] - r["obj_highs"]) for r in rows), w["gap"], time.time() - t0), flush=True)
