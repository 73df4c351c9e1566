"""GPU: the primal phase 1 of the LP engine and the switch between its simplex methods (bslv_lpq_set_method: DUAL, the default;
PRIMAL; REPAIR), against the CPU oracle's primal simplex (oracle/lp_dense.c primal_simplex, olp.solve(0)) and HiGHS.

The random LPs are in GLPK's row / column model with all five bound types (f l u d s); every set holds one LP that is infeasible
by construction (two rows with the same coefficients and bounds that contradict each other), one that is unbounded by construction
(a free column with a cost and no row) and, mostly, LPs that are feasible by construction around a point x0 -- whose standard basis
is almost never primal feasible, so phase 1 has work.  Optimal values: 1e-9 relative (the project's bound for primal steps against
the oracle, tests/test_lp_gpu.py RTOL).  The seeds were checked on the CPU: the oracle and HiGHS agree on every LP of every set.

Run as a program (`python tests/test_lp_primal_gpu.py child M N`) it solves the cold-start set of that shape and prints statuses
and objective values as one JSON line: the poisoned-allocation test starts it that way, once per fill byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bensolve_amd.lp import LpEngine
from lp_cases import random_lp, highs, oracle_primal, check_optimality_conditions

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SHAPES = [(6, 5), (17, 23), (40, 70)]      # 23 pads to ld = 32; 70 crosses one wave of 64 columns and one ld step
SEEDS = {(6, 5): 101, (17, 23): 102, (40, 70): 103}
NLP = 40
DUAL, PRIMAL, REPAIR = 0, 1, 2
OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED = 4, 0, 1, 3
E_ARG = 2
NONE = np.zeros((1, 0))


# ---- the LPs (random_lp and the yardsticks: tests/lp_cases.py) ----------------------------------------------------------
def lp_set(M, N):
    rng = np.random.default_rng(SEEDS[(M, N)])
    kinds = ["infeasible", "unbounded"] + ["wild" if t % 5 == 4 else "feasible" for t in range(2, NLP)]
    return [random_lp(M, N, rng, k) for k in kinds]


_REF = {}


def references(M, N):
    """the LPs of a shape with the oracle's and HiGHS' answers, computed once and shared"""
    if (M, N) not in _REF:
        rows = []
        for A, lo, up, cost in lp_set(M, N):
            so, zo = oracle_primal(A, lo, up, cost)
            sh, zh = highs(A, lo, up, cost)
            rows.append(dict(A=A, lo=lo, up=up, cost=cost, st=so, obj=zo, st_highs=sh, obj_highs=zh))
        _REF[(M, N)] = rows
    return _REF[(M, N)]


def cold_solve(A, lo, up, cost, method, details=False):
    """one LP from the standard basis, in place, under `method`"""
    M, N = A.shape
    eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 2)
    assert eng.set_method(method) == 0
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], NONE, NONE)
    out = dict(st=int(st[0]), iters=int(it[0]), obj=float(eng.obj([0])[0]), stats=eng.last_stats())
    if details:
        out["prim"] = eng.primal([0], 0, M + N)[0]
        out["dual"] = eng.dual([0], 0, M + N)[0]
    eng.close()
    return out


# ---- 1. cold start under PRIMAL --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SHAPES)
def test_cold_start_under_primal_matches_oracle_and_highs(oracle, M, N):
    ref = references(M, N)
    assert ref[0]["st"] == INFEASIBLE and ref[1]["st"] == UNBOUNDED                 # the two built on purpose
    assert sum(r["st"] == OPTIMAL for r in ref) >= NLP // 2
    p1_lps = p1_its = 0
    for t, r in enumerate(ref):
        assert r["st"] == r["st_highs"], (t, r["st"], r["st_highs"])                # (the yardsticks agree: checked when the seeds were chosen)
        got = cold_solve(r["A"], r["lo"], r["up"], r["cost"], PRIMAL, details=True)
        print("lp %d: status %d (oracle %d, HiGHS %d) iters %d obj %r (oracle %r) phase 1: %s" % (t, got["st"], r["st"], r["st_highs"], got["iters"], got["obj"], r["obj"],
              {k: v for k, v in got["stats"].items() if k.startswith("phase1")}))
        assert got["st"] == r["st"], (t, got["st"], r["st"])
        p1_lps += got["stats"]["phase1_lps"]
        p1_its += got["stats"]["phase1_iterations"]
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(got["obj"], r["obj"], rtol=RTOL, atol=1e-9, err_msg="lp %d" % t)
            np.testing.assert_allclose(got["obj"], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="lp %d (HiGHS)" % t)
            check_optimality_conditions(r["A"], r["lo"], r["up"], r["cost"], got["obj"], got["prim"], got["dual"], (M, N, t))
    assert p1_lps > 0 and p1_its > 0, (p1_lps, p1_its)


# ---- a boxed model for the warm starts: feasible around x0, every row and column with two bounds -----------------------------
def boxed_model(M, N, seed):
    rng = np.random.default_rng(seed)
    A = np.round(rng.normal(size=(M, N)) * 3) / 2
    A[rng.random((M, N)) < 0.4] = 0.0
    for i in range(M):
        if np.count_nonzero(A[i]) < 2:      # (no row the presolve would fold)
            A[i, rng.choice(N, 2, replace=False)] = 1.0
    x0 = np.round(rng.normal(size=N) * 2)
    r0 = A @ x0
    lo = np.concatenate([r0 - rng.integers(1, 4, size=M), x0 - rng.integers(1, 4, size=N)]).astype(float)
    up = np.concatenate([r0 + rng.integers(1, 4, size=M), x0 + rng.integers(1, 4, size=N)]).astype(float)
    cost = np.concatenate([[0.0], np.round(rng.normal(size=N) * 3)])
    return A, lo, up, cost


# ---- 2. a warm start that is infeasible on both sides -------------------------------------------------------------------------
def test_warm_start_infeasible_on_both_sides(oracle):
    M, N = 17, 23
    A, lo, up, cost = boxed_model(M, N, 202)
    eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 4)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], NONE, NONE)
    assert st[0] == OPTIMAL
    prim, dual = eng.primal([0], 0, M + N)[0], eng.dual([0], 0, M + N)[0]
    # a row variable that is nonbasic on a bound with |d| > 1e-3 loses that bound (a row: a column with a cost would get an
    # artificial bound in its place and the dual simplex could start); a basic variable well inside its bounds gets an upper
    # bound below its value.  Of the pairs the returned solution offers, the first whose LP the oracle solves to optimality.
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
                chosen = (kn, kb, lo2, up2, zo)
                break
        if chosen:
            break
    assert chosen, "no pair of changes leaves a solvable LP"
    kn, kb, lo2, up2, zo = chosen
    eng.set_bounds(lo2, up2)
    assert eng.get_method() == DUAL
    st, _ = eng.solve_batch([0], [1], NONE, NONE)
    assert st[0] == UNDEFINED                       # the default: the dual simplex cannot start there
    for method, dst in ((REPAIR, 2), (PRIMAL, 3)):
        assert eng.set_method(method) == 0
        st, it = eng.solve_batch([0], [dst], NONE, NONE)
        stats = eng.last_stats()
        z = eng.obj([dst])[0]
        print("method %d: status %d iters %d obj %r (oracle %r) %s" % (method, st[0], it[0], z, zo, stats))
        assert st[0] == OPTIMAL, (method, st)
        np.testing.assert_allclose(z, zo, rtol=RTOL, atol=1e-9)
        assert stats["phase1_lps"] == 1, stats
        check_optimality_conditions(A, lo2, up2, cost, z, eng.primal([dst], 0, M + N)[0], eng.dual([dst], 0, M + N)[0], method)
    eng.close()


# ---- 3. a mixed batch under REPAIR ------------------------------------------------------------------------------------------
def _row_range_engine(seed, slots):
    """the boxed model with per-LP bounds on all its rows, slot 0 solved for the bounds of the model"""
    M, N = 17, 23
    A, lo, up, cost = boxed_model(M, N, seed)
    eng = LpEngine(M, N, A, lo, up, cost, 0, M, slots)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], lo[None, :M], up[None, :M])
    assert st[0] == OPTIMAL
    return eng, M, N, lo, up


def _results(eng, dst, M, N, st, it):
    return dict(st=np.array(st), it=np.array(it), obj=eng.obj(dst), prim=eng.primal(dst, 0, M + N), dual=eng.dual(dst, 0, M + N))


def _assert_identical(a, b, tag):
    for k in ("st", "it", "obj", "prim", "dual"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k, a[k], b[k])


def test_mixed_batch_under_repair_equals_its_lps_alone():
    B = 16
    eng, M, N, lo, up = _row_range_engine(303, 2 * B + 1)
    dual = eng.dual([0], 0, M)[0]
    nonbasic = [k for k in range(M) if abs(dual[k]) > 1e-3]
    assert nonbasic
    rng = np.random.default_rng(5)
    vlo, vup = np.tile(lo[:M], (B, 1)), np.tile(up[:M], (B, 1))
    for b in range(B):
        vlo[b] -= rng.integers(0, 2, size=M); vup[b] += rng.integers(0, 2, size=M)      # other boxes: the dual simplex starts
        if b % 2:                                                                       # and a bound gone from under a reduced cost: it cannot
            k = nonbasic[(b // 2) % len(nonbasic)]
            if dual[k] > 0: vlo[b, k] = -np.inf
            else: vup[b, k] = np.inf
    assert eng.set_method(REPAIR) == 0
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, vlo, vup)
    stats = eng.last_stats()
    print("batch: statuses %s iters %s %s" % (st, it, stats))
    assert 0 < stats["phase1_lps"] < B, stats       # some need phase 1, some none
    assert np.all(st != UNDEFINED), st              # a result, not a retry
    together = _results(eng, dst, M, N, st, it)
    alone = dict(st=[], it=[])
    dst1 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    for b in range(B):
        s1, i1 = eng.solve_batch([0], [dst1[b]], vlo[b:b + 1], vup[b:b + 1])
        alone["st"].append(s1[0]); alone["it"].append(i1[0])
    _assert_identical(together, _results(eng, dst1, M, N, alone["st"], alone["it"]), "batch against single LPs")
    eng.close()


# ---- 4. ties --------------------------------------------------------------------------------------------------------------
def test_hypercube_with_ties_terminates_under_primal(oracle):
    n, rows = 12, 6
    rng = np.random.default_rng(7)
    A = np.zeros((rows, n))
    for i in range(rows):
        A[i, rng.choice(n, 4, replace=False)] = 1.0
    A[:, 0] = 1.0                                    # the variable of the objective helps every cover row
    lo = np.concatenate([np.ones(rows), np.zeros(n)])
    up = np.concatenate([np.full(rows, np.inf), np.ones(n)])
    cost = np.zeros(n + 1); cost[1] = 1.0
    so, zo = oracle_primal(A, lo, up, cost)
    assert so == OPTIMAL
    got = cold_solve(A, lo, up, cost, PRIMAL)
    print(got)
    assert got["st"] == OPTIMAL and got["iters"] < 50 * (rows + n) + 1000
    np.testing.assert_allclose(got["obj"], zo, rtol=RTOL, atol=1e-9)


# ---- 5. the default is untouched --------------------------------------------------------------------------------------------
def test_default_method_is_dual_and_a_detour_leaves_no_trace():
    B = 12
    rng = np.random.default_rng(11)
    out = []
    for detour in (False, True):
        eng, M, N, lo, up = _row_range_engine(303, 2 * B + 2)
        assert eng.get_method() == DUAL
        if detour:
            assert eng.set_method(PRIMAL) == 0 and eng.get_method() == PRIMAL
            st, _ = eng.solve_batch([0], [2 * B + 1], lo[None, :M], up[None, :M])       # a solve in another slot
            assert st[0] == OPTIMAL
            assert eng.set_method(DUAL) == 0 and eng.get_method() == DUAL
        if not out:
            vlo = np.tile(lo[:M], (B, 1)) - rng.integers(0, 3, size=(B, M))
            vup = np.tile(up[:M], (B, 1)) + rng.integers(0, 3, size=(B, M))
        dst = np.arange(1, B + 1, dtype=np.int32)
        st, it = eng.solve_batch(np.zeros(B, np.int32), dst, vlo, vup)
        assert np.all(st == OPTIMAL) and eng.last_stats()["phase1_lps"] == 0
        out.append(_results(eng, dst, M, N, st, it))
        eng.close()
    _assert_identical(out[0], out[1], "fresh engine against one after a detour through PRIMAL")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    M, N = 6, 5
    A, lo, up, cost = boxed_model(M, N, 404)
    eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 2)
    assert eng.set_method(7) == E_ARG and eng.set_method(-1) == E_ARG and eng.get_method() == DUAL
    eng.close()
    monkeypatch.setenv("BSLV_LP_REV", "1")
    monkeypatch.setenv("BSLV_LP_METHOD", "primal")          # ignored by an engine that comes up in the revised form
    eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 2)
    eng.lib.bslv_lpq_is_revised.argtypes = [__import__("ctypes").c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == 1 and eng.get_method() == DUAL
    assert eng.set_method(PRIMAL) == E_ARG and eng.set_method(REPAIR) == E_ARG and eng.set_method(DUAL) == 0
    eng.lib.bslv_last_error.restype = __import__("ctypes").c_char_p
    assert b"revised" in eng.lib.bslv_last_error()
    eng.close()
    monkeypatch.delenv("BSLV_LP_REV")
    monkeypatch.setenv("BSLV_LP_METHOD", "repair")
    eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 2)
    assert eng.get_method() == REPAIR
    eng.close()


# ---- 7. poisoned allocations -------------------------------------------------------------------------------------------------
def _child(M, N):
    rows = []
    for A, lo, up, cost in lp_set(M, N):
        got = cold_solve(A, lo, up, cost, PRIMAL)
        rows.append([got["st"], got["obj"].hex() if got["st"] == OPTIMAL else None])
    print(json.dumps(dict(fill=os.environ.get("BSLV_FILL"), rows=rows)))


def test_cold_start_does_not_depend_on_the_fill_byte():
    out = []
    for fill in ("0x00", "0x7F"):
        env = dict(os.environ, BSLV_FILL=fill)
        env.pop("BSLV_ALLOC_LOG", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "17", "23"], env=env, capture_output=True, text=True, timeout=300)
        assert "Memory access fault" not in p.stderr, "fill %s: %s" % (fill, p.stderr[-800:])
        assert p.returncode == 0, "fill %s: rc %d\n%s" % (fill, p.returncode, p.stderr[-1500:])
        row = json.loads(p.stdout.strip().splitlines()[-1])
        assert row["fill"] == fill
        out.append(row["rows"])
    assert len(out[0]) == NLP and out[0] == out[1]
    assert [r[0] for r in out[0]] == [r["st"] for r in references(17, 23)]


# ---- 8. through the program --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["primal", "repair"])
@pytest.mark.parametrize("ex", ["ex01", "ex05"])
def test_cli_under_the_method_matches_the_hybrid_goldens(tmp_path, ex, method):
    from test_cli_gpu import CLI, EXDIR, EX_TOL, GOLD, _gold_rows, read_img      # (the comparison of test_cli_all_phases_match_hybrid_goldens)
    base = os.path.join(tmp_path, ex)
    r = subprocess.run([CLI, os.path.join(EXDIR, ex + ".vlp"), "-m", "2", "-B", "64", "-o", base], env=dict(os.environ, BSLV_LP_METHOD=method),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for side in ("p", "d"):
        t, X, _ = read_img(base + "_img_%s.sol" % side)
        gt, gX = _gold_rows(GOLD["%s/%s_type" % (ex, side)], GOLD["%s/%s" % (ex, side)])
        assert np.array_equal(t, gt), (ex, side, r.stdout)
        np.testing.assert_allclose(X, gX, rtol=EX_TOL, atol=EX_TOL)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "child":
        _child(int(sys.argv[2]), int(sys.argv[3]))
