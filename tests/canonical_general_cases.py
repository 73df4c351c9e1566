"""Cases for the canonical-dual tests on GENERAL models (tests/test_lp_canonical_general_gpu.py): the sets of lp_cases.general_set
with TIES put into their LPs, a direction for the per-LP bounds, and the EXPECTED canonical dual from scipy's HiGHS.  No GPU in here,
and nothing of oracle/ except through lp_cases (which LPs both yardsticks call OPTIMAL).

A P2(v) model (tests/canonical_cases.py) has only upper bounds on its per-LP range and no bounds on its columns, so it reaches half
of the tie phase (tie_once, bensolve_amd/csrc/lp_engine.hip).  Here the per-LP range holds rows ("a") or columns ("b") of all five
bound types, and a tie is made where there was none: the LP is solved, up to TIES per-LP variables that lie strictly inside their
bounds get ONE FINITE bound moved onto their value (boxed variables: the lower and the upper bound in turn) -- the optimum stays what it
was, and each of them is a basic variable on a bound, lower or upper.  No infinite side becomes finite (general_set's contract).

The canonical dual for a direction d is the dual the LP has for the per-LP bounds lo + t d, up + t d (finite sides only) for all small
t > 0 (include/bslv_hip.h, bslv_lpq_set_canonical).  Keep rule, as canonical_cases.py's: the full dual vector (M + N entries, rows
first) is the same at T1 and T2 to SAME_W, the optimal value is linear through t = 0, and the vector -- with the primal solution of
t = 0 -- passes lc.assert_certified for the LP at t = 0 (in np.longdouble, with no allowance for an oracle's gap): it is still optimal
at 0, and its signs are lc.certify's.  The others are dropped and counted.

HiGHS solves every LP in the form with row variables, [A -I](x, r) = 0 with bounds on x and r: the row duals are the marginals of
the equalities, the column duals c - A' lambda.

tied_set     the kept cases of one set and arrangement with their expected duals; "a": d_k = 1 + hash01(k), "b": that times (-1)^k
exit_set     arrangement "a" with the mixed-sign direction: the shifted LP of every tied LP is INFEASIBLE at T1 and at T2 (rows 0 and 1
             have equal coefficients, both get tied on the same value, one from below and one from above, and move apart), so the
             tie phase has to end without an entering candidate

Run as a program (`python tests/canonical_general_cases.py`) it prints the table of every set."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import canonical_cases as cc
import lp_cases as lc
from canonical_cases import T1, T2, SAME_W, OPT_TOL
from lp_cases import OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED, NLP

REQUIRED = [(16, 17), (32, 65)]             # ld 16 against 32, one wave of columns against two
EXTRA = [(15, 16), (31, 64)]                # their neighbours: run as well, they meet the conditions
SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65)]
EXIT_SHAPES = [(16, 17), (32, 65), (24, 1536)]
TIES = 3
INSIDE = 1e-6                               # "strictly inside its bounds"
DEGENERATE = 1e-6                           # the expected dual on a tied variable
MIN_KEPT = 10


def positive_direction(cnt):
    return np.array([1.0 + cc.hash01(k) for k in range(cnt)])


def mixed_direction(cnt):
    return np.array([(1.0 + cc.hash01(k)) * (-1.0) ** k for k in range(cnt)])


def solve_rowform(A, lo, up, cost):
    """(status in the engine's numbering, optimal value, primal, dual) from HiGHS on min c.x s.t. A x - r = 0, lo <= (r, x) <= up;
    the vectors over rows then columns as the engine returns them"""
    from scipy.optimize import linprog
    M, N = A.shape
    kw = dict(A_eq=np.hstack([A, -np.eye(M)]), b_eq=np.zeros(M),
              bounds=[(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(np.concatenate([lo[M:], lo[:M]]), np.concatenate([up[M:], up[:M]]))])
    c = np.concatenate([cost[1:], np.zeros(M)])
    res = linprog(c, method="highs", **kw)
    if res.status != 0:                     # (lc.highs: HiGHS' presolve reports 'infeasible' for 'infeasible or unbounded')
        res = linprog(c, method="highs", options={"presolve": False}, **kw)
    st = {0: OPTIMAL, 2: INFEASIBLE, 3: UNBOUNDED}.get(res.status, UNDEFINED)
    if st != OPTIMAL:
        return st, None, None, None
    lam = np.asarray(res.eqlin.marginals, float)
    x = np.asarray(res.x, float)
    return st, res.fun + cost[0], np.concatenate([x[N:], x[:N]]), np.concatenate([lam, cost[1:] - A.T @ lam])


def shifted(lo, up, first, d, t):
    """the bounds with the finite sides of the per-LP range moved by t d"""
    l, u = lo.copy(), up.copy()
    k = slice(first, first + len(d))
    l[k] = np.where(np.isfinite(lo[k]), lo[k] + t * d, lo[k])
    u[k] = np.where(np.isfinite(up[k]), up[k] + t * d, up[k])
    return l, u


def tie(lo, up, prim, first, cnt, turn):
    """(lo, up, ties, turn) with up to TIES ties put into one LP: the first per-LP variables, in the order of the range, that lie
    strictly inside their bounds and have a finite one; ties is a list of (variable, "lo" or "up"); `turn` counts the boxed variables
    tied so far (even: the lower bound moves, odd: the upper one)"""
    lo, up, ties = lo.copy(), up.copy(), []
    for k in range(first, first + cnt):
        if len(ties) == TIES:
            break
        flo, fup = np.isfinite(lo[k]), np.isfinite(up[k])
        if lo[k] == up[k] or not (flo or fup):
            continue
        if (flo and prim[k] < lo[k] + INSIDE) or (fup and prim[k] > up[k] - INSIDE):
            continue
        if flo and fup:
            side = "lo" if turn % 2 == 0 else "up"
            turn += 1
        else:
            side = "lo" if flo else "up"
        (lo if side == "lo" else up)[k] = prim[k]
        ties.append((k, side))
    return lo, up, ties, turn


def _tied_lps(M, N, arr):
    """general_set's LPs that both yardsticks call OPTIMAL, each solved by HiGHS and tied: rows of dict(t, lo, up, ties, z, prim)"""
    s = lc.general_set(M, N, arr)
    ref, _ = lc.assert_references_agree(M, N, arr)
    first, cnt = s["var_first"], s["var_cnt"]
    rows, turn = [], 0
    for t, (lo, up) in enumerate(s["lps"]):
        if not (ref[t]["st"] == ref[t]["st_highs"] == OPTIMAL):
            continue
        st, z, prim, _ = solve_rowform(s["A"], lo, up, s["cost"])
        assert st == OPTIMAL and abs(z - ref[t]["obj"]) <= OPT_TOL * (1.0 + abs(z)), (M, N, arr, t, st, z, ref[t]["obj"])
        tlo, tup, ties, turn = tie(lo, up, prim, first, cnt, turn)
        assert np.array_equal(np.isfinite(tlo), np.isfinite(lo)) and np.array_equal(np.isfinite(tup), np.isfinite(up))
        rows.append(dict(t=t, lo=tlo, up=tup, ties=ties, z=z, prim=prim))
    return s, rows


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


_TIED, _EXIT = {}, {}


def tied_set(M, N, arr):
    """The kept cases of general_set(M, N, arr) with ties, computed once per process and never changed.  A dict: the model (A, lo, up,
    cost, var_first, var_cnt, tr, tc), dir, perm, and per kept case lps (its LP of general_set), vlo / vup (the tied bounds of the
    per-LP range), bounds (the full lo, up), ties, z, prim (HiGHS at t = 0), dual (the expected canonical dual, M + N), degenerate;
    candidates and dropped count the LPs the keep rule saw and turned away."""
    key = (M, N, arr)
    if key in _TIED:
        return _TIED[key]
    s, rows = _tied_lps(M, N, arr)
    first, cnt = s["var_first"], s["var_cnt"]
    d = positive_direction(cnt) if arr == "a" else mixed_direction(cnt)
    kept = []
    for r in rows:
        if not r["ties"]:
            continue
        s1, z1, _, y1 = solve_rowform(s["A"], *shifted(r["lo"], r["up"], first, d, T1), s["cost"])
        s2, z2, _, y2 = solve_rowform(s["A"], *shifted(r["lo"], r["up"], first, d, T2), s["cost"])
        if s1 != OPTIMAL or s2 != OPTIMAL or np.abs(y1 - y2).max() > SAME_W:
            continue
        if abs((z1 - r["z"]) - 2.0 * (z2 - r["z"])) > OPT_TOL * (1.0 + abs(r["z"])):          # linear through t = 0
            continue
        cert = lc.certify(s["A"], r["lo"], r["up"], s["cost"], OPTIMAL, r["z"], r["prim"], y2)
        try:
            lc.assert_certified(cert, r["z"], 0.0, (M, N, arr, r["t"]))
        except AssertionError:
            continue
        kept.append(dict(r, dual=y2, degenerate=any(abs(y2[k]) > DEGENERATE for k, _ in r["ties"])))
    sl = slice(first, first + cnt)
    out = dict(M=M, N=N, arr=arr, A=s["A"], lo=s["lo"], up=s["up"], cost=s["cost"], tr=s["tr"], tc=s["tc"], var_first=first, var_cnt=cnt,
               dir=d, perm=s["perm"], vlo0=s["vlo"][0], vup0=s["vup"][0], lps=np.array([r["t"] for r in kept], np.int32),
               vlo=np.array([r["lo"][sl] for r in kept]), vup=np.array([r["up"][sl] for r in kept]), bounds=[(r["lo"], r["up"]) for r in kept],
               ties=[r["ties"] for r in kept], z=np.array([r["z"] for r in kept]), prim=np.array([r["prim"] for r in kept]),
               dual=np.array([r["dual"] for r in kept]), degenerate=np.array([r["degenerate"] for r in kept], bool),
               candidates=len(rows), dropped=len(rows) - len(kept))
    _TIED[key] = _freeze(out)
    return out


def tie_kinds(c):
    """what the ties of a set's kept cases are: counts of ties on a lower and on an upper bound, of tied boxed ('d') columns, of tied
    per-LP columns, and of each of these with a non-zero expected dual (the ties that decide the canonical dual)"""
    M = c["M"]
    n = dict(lower=0, upper=0, boxed_col=0, col=0, lower_nz=0, upper_nz=0, boxed_col_nz=0, col_nz=0)
    for ties, y in zip(c["ties"], c["dual"]):
        for k, side in ties:
            names = ["lower" if side == "lo" else "upper"]
            if k >= M:
                names.append("col")
                if c["tc"][k - M] == "d":
                    names.append("boxed_col")
            for name in names:
                n[name] += 1
                n[name + "_nz"] += int(abs(y[k]) > DEGENERATE)
    return n


def check_tied_set(c):
    """the conditions one set has to meet before anything is compared against it"""
    kept = len(c["lps"])
    assert kept >= MIN_KEPT, "only %d cases kept" % kept
    assert 2 * int(c["degenerate"].sum()) >= kept, "%d of %d kept cases are degenerate" % (int(c["degenerate"].sum()), kept)


def check_all_sets(sets):
    """... and the required sets together: a tie on a lower and one on an upper bound, a tied boxed column, and in arrangement "b" a
    tied per-LP column -- each of them with a non-zero expected dual, so that the tie decides what the engine has to return"""
    tot = {}
    for c in sets:
        for k, v in tie_kinds(c).items():
            tot[k] = tot.get(k, 0) + v
    assert tot["lower_nz"] > 0 and tot["upper_nz"] > 0 and tot["boxed_col_nz"] > 0, tot
    colb = sum(tie_kinds(c)["col_nz"] for c in sets if c["arr"] == "b")
    assert colb > 0, tot
    return tot


def exit_set(M, N):
    """general_set(M, N, "a") tied as in tied_set, with the mixed-sign direction and no keep rule: every LP both yardsticks call
    OPTIMAL, with the status HiGHS gives its shifted LP at T1 and at T2.  A dict: the model, dir, lps, vlo / vup (NLP rows: the tied
    bounds of the OPTIMAL LPs, general_set's of the others), bounds, optimal (NLP flags), z, shifted_status (per OPTIMAL LP, (T1, T2))."""
    if (M, N) in _EXIT:
        return _EXIT[(M, N)]
    s, rows = _tied_lps(M, N, "a")
    first, cnt = s["var_first"], s["var_cnt"]
    d = mixed_direction(cnt)
    vlo, vup = s["vlo"].copy(), s["vup"].copy()
    bounds = [(lo.copy(), up.copy()) for lo, up in s["lps"]]
    optimal = np.zeros(NLP, bool)
    stats = []
    for r in rows:
        t = r["t"]
        optimal[t] = True
        vlo[t], vup[t] = r["lo"][first:first + cnt], r["up"][first:first + cnt]
        bounds[t] = (r["lo"], r["up"])
        stats.append(tuple(solve_rowform(s["A"], *shifted(r["lo"], r["up"], first, d, tt), s["cost"])[0] for tt in (T1, T2)))
    z = np.full(NLP, np.nan)
    z[[r["t"] for r in rows]] = [r["z"] for r in rows]
    out = dict(M=M, N=N, A=s["A"], lo=s["lo"], up=s["up"], cost=s["cost"], var_first=first, var_cnt=cnt, dir=d, vlo0=s["vlo"][0], vup0=s["vup"][0],
               lps=np.array([r["t"] for r in rows], np.int32), vlo=vlo, vup=vup, bounds=bounds, optimal=optimal, z=z, ties=[r["ties"] for r in rows],
               shifted_status=stats)
    _EXIT[(M, N)] = _freeze(out)
    return out


def table_line(c):
    n = tie_kinds(c)
    return ("canonical_general_cases M %d N %d arr %s: candidates %d kept %d degenerate %d dropped %d; ties lower %d (%d non-zero) upper %d (%d) "
            "boxed columns %d (%d) columns %d (%d)" % (c["M"], c["N"], c["arr"], c["candidates"], len(c["lps"]), int(c["degenerate"].sum()), c["dropped"],
                                                       n["lower"], n["lower_nz"], n["upper"], n["upper_nz"], n["boxed_col"], n["boxed_col_nz"], n["col"], n["col_nz"]))


if __name__ == "__main__":
    import time
    sets = []
    for M, N in SHAPES:
        for arr in ("a", "b"):
            t0 = time.time()
            c = tied_set(M, N, arr)
            print(table_line(c) + " (%.1f s)" % (time.time() - t0), flush=True)
            check_tied_set(c)
            if (M, N) in REQUIRED:
                sets.append(c)
    print("required sets together: %s" % check_all_sets(sets))
    for M, N in EXIT_SHAPES:
        t0 = time.time()
        e = exit_set(M, N)
        bad = [st for st in e["shifted_status"] if st != (INFEASIBLE, INFEASIBLE)]
        print("canonical_general_cases exit M %d N %d: %d OPTIMAL LPs, shifted LP infeasible at T1 and T2 in %d (%.1f s)" % (
            M, N, len(e["lps"]), len(e["lps"]) - len(bad), time.time() - t0), flush=True)
        assert not bad, bad
