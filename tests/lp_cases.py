"""LPs in GLPK's row / column model with all five bound types (f l u d s), the two CPU yardsticks for them (scipy's HiGHS and the
oracle's primal simplex, oracle/lp_dense.c) and a certificate of optimality that needs no solver.  No GPU in here.

random_lp                      one LP: feasible around a point, infeasible or unbounded by construction, or "wild"
general_set                    one model and 16 LPs that differ only in the bounds of a per-LP range (tests/test_lp_general_gpu.py)
objective_set                  the model of a shape with a zero cost and 3 x 16 cost vectors over a range of variables, rows included
                               (tests/test_lp_obj_general_gpu.py); unbounded_objective_set: some of them unbounded
certify / assert_certified     residuals of a returned solution in np.longdouble, and the project's bounds on them

Run as a program (`python tests/lp_cases.py [M N ...]`) it solves every LP of every set with both yardsticks, asserts that they agree
and prints the oracle's residuals per shape: the check made when the seeds were chosen.  `python tests/lp_cases.py obj [M N ...]` does
the same for the objective sets, per shape and cost range."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bensolve_amd.lp import bounds_from_types

RTOL = 1e-9
OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED = 4, 0, 1, 3
LD = np.longdouble


def _bounds(types, lb, ub):
    lo, up = bounds_from_types(np.array(list(types)), lb, ub)
    return lo, up


def random_lp(M, N, rng, kind, bounded=False, parts=False):
    """(A, lo, up, cost) of one LP: lo / up over the M row variables then the N columns, cost[0] the constant shift.
    bounded: a "feasible" LP always gets costs that pull no column where it has no bound (without it: with probability 0.7).
    parts: also returns (x0, row types, column types), the point the bounds were built around and the bound types."""
    A = np.round(rng.normal(size=(M, N)) * 3) / 2
    A[rng.random((M, N)) < 0.4] = 0.0
    for i in range(M):                      # no empty row
        if not A[i].any():
            A[i, rng.integers(N)] = 1.0
    x0 = np.round(rng.normal(size=N) * 2)
    tr = rng.choice(list("fluds"), size=M, p=[.1, .3, .3, .2, .1])
    tc = rng.choice(list("fluds"), size=N, p=[.15, .4, .1, .25, .1])
    cost = np.concatenate([[float(rng.integers(-2, 3))], np.round(rng.normal(size=N) * 3)])
    if kind == "wild":                      # bounds that know nothing of each other: feasible, infeasible or unbounded as it comes
        rl = np.round(rng.normal(size=M) * 2)
        cl = np.round(rng.normal(size=N) * 2)
        ru, cu = rl + rng.integers(0, 4, size=M), cl + rng.integers(0, 4, size=N)
    else:                                   # feasible: x0 lies within all of them
        if kind == "unbounded":
            A[:, 0] = 0.0
            for i in range(M):
                if not A[i].any():
                    A[i, 1 + rng.integers(N - 1)] = 1.0
        r0 = A @ x0
        rl, cl = r0 - rng.integers(0, 3, size=M), x0 - rng.integers(0, 3, size=N)
        ru, cu = r0 + rng.integers(0, 3, size=M), x0 + rng.integers(0, 3, size=N)
        rl, cl = np.where(tr == "s", r0, rl), np.where(tc == "s", x0, cl)
        ru, cu = np.where((tr == "d") & (ru == rl), rl + 1, ru), np.where((tc == "d") & (cu == cl), cl + 1, cu)
    if kind == "feasible" and (bounded or rng.random() < 0.7):      # most of them bounded as well: no cost pulls a column where it has no bound
        c = cost[1:]
        c[:] = np.where(tc == "f", 0.0, np.where(tc == "l", np.abs(c), np.where(tc == "u", -np.abs(c), c)))
    rlo, rup = _bounds(tr, rl, ru)
    clo, cup = _bounds(tc, cl, cu)
    if kind == "unbounded":                 # a free column with a cost and no row
        clo[0], cup[0], cost[1] = -np.inf, np.inf, 1.0
    if kind == "infeasible":                # two rows that contradict each other
        A[1] = A[0]
        rlo[0], rup[0] = 5.0, np.inf
        rlo[1], rup[1] = -np.inf, 4.0
    out = (A, np.concatenate([rlo, clo]), np.concatenate([rup, cup]), cost)
    return out + (x0, tr, tc) if parts else out


# ---- the yardsticks --------------------------------------------------------------------------------------------------------
def highs(A, lo, up, cost):
    """(status in the engine's numbering, optimal value) from scipy's HiGHS"""
    from scipy.optimize import linprog
    M, N = A.shape
    Aub, bub, Aeq, beq = [], [], [], []
    for i in range(M):
        if lo[i] == up[i]:
            Aeq.append(A[i]); beq.append(lo[i])
        else:
            if np.isfinite(up[i]): Aub.append(A[i]); bub.append(up[i])
            if np.isfinite(lo[i]): Aub.append(-A[i]); bub.append(-lo[i])
    kw = dict(A_ub=np.array(Aub) if Aub else None, b_ub=bub if Aub else None, A_eq=np.array(Aeq) if Aeq else None, b_eq=beq if Aeq else None,
              bounds=[(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(lo[M:], up[M:])])
    res = linprog(cost[1:], method="highs", **kw)
    if res.status != 0:                     # HiGHS' presolve reports 'infeasible' for 'infeasible or unbounded'
        res = linprog(cost[1:], method="highs", options={"presolve": False}, **kw)
    st = {0: OPTIMAL, 2: INFEASIBLE, 3: UNBOUNDED}.get(res.status, UNDEFINED)
    return st, (res.fun + cost[0]) if st == OPTIMAL else None


def oracle_solution(A, lo, up, cost):
    """the oracle's primal method from the standard basis: (status, optimal value, primal, dual); the vectors over rows then columns"""
    import oracle_api
    M, N = A.shape
    olp = oracle_api.OracleLP(A, lo, up, cost)
    st = olp.solve(0)
    z = prim = dual = None
    if st == OPTIMAL:
        z, prim, dual = olp.obj(), olp.primal(0, M + N), olp.dual(0, M + N)
    olp.close()
    return st, z, prim, dual


def oracle_primal(A, lo, up, cost):
    """the oracle's primal method from the standard basis: (status, optimal value)"""
    return oracle_solution(A, lo, up, cost)[:2]


def check_optimality_conditions(A, lo, up, cost, z, prim, dual, tag):
    """of the model as given (tests/test_lp_gpu.py test_presolve_keeps_the_model_of_the_caller_primal_and_dual): r = A x within the
    bounds, d = c - A' lambda, every non-zero dual on a bound of the matching sign"""
    M, N = A.shape
    x, r, lam, d = prim[M:], prim[:M], dual[:M], dual[M:]
    np.testing.assert_allclose(r, A @ x, atol=1e-9, err_msg=str(tag))
    np.testing.assert_allclose(z, cost[0] + cost[1:] @ x, atol=1e-9, err_msg=str(tag))
    np.testing.assert_allclose(d, cost[1:] - A.T @ lam, atol=1e-8, err_msg=str(tag))
    assert np.all(prim >= lo - 1e-8) and np.all(prim <= up + 1e-8), tag
    for k in range(M + N):
        if abs(dual[k]) > 1e-9:
            at_lo, at_up = abs(prim[k] - lo[k]) < 1e-7, abs(prim[k] - up[k]) < 1e-7
            assert (dual[k] > 0 and at_lo) or (dual[k] < 0 and at_up) or (at_lo and at_up), (tag, k, dual[k], prim[k], lo[k], up[k])


# ---- the certificate -------------------------------------------------------------------------------------------------------
TOL_ROWS, TOL_FEAS, TOL_DJ, TOL_SIDE, DUAL_ZERO = 1e-9, 1e-8, 1e-8, 1e-7, 1e-9      # check_optimality_conditions' figures


def certify(A, lo, up, cost, status, z, prim, dual):
    """Worst residual of each kind of a solution returned as OPTIMAL, from the model and the returned vectors alone, in np.longdouble:
      rows   |r - A x|, the returned row values against the product
      feas   how far a variable is outside [lo, up], divided by 1 + |bound|
      dj     |d - (c - A' lambda)|
      side   for every dual with |.| > 1e-9: the distance of its variable from the bound of the dual's sign (> 0: lower, < 0: upper;
             inf where that bound does not exist)
      gap    the larger of |D - P| and |P - z|: P = c0 + c.x, D = c0 + the sum of dual times the bound of its sign (the dual
             objective: with r = A x and d = c - A' lambda, c.x = lambda.r + d.x, and complementarity puts every term on its bound)
    Any other status: None."""
    if status != OPTIMAL:
        return None
    M, N = A.shape
    Al, c = A.astype(LD), np.asarray(cost, LD)
    p, y = np.asarray(prim, LD), np.asarray(dual, LD)
    lo, up = np.asarray(lo, np.float64), np.asarray(up, np.float64)
    x, r, lam, d = p[M:], p[:M], y[:M], y[M:]
    out = {}
    out["rows"] = float(np.abs(r - Al @ x).max())
    with np.errstate(invalid="ignore"):
        below = np.where(np.isfinite(lo), (lo.astype(LD) - p) / (1 + np.abs(np.where(np.isfinite(lo), lo, 0.0))), -np.inf)
        above = np.where(np.isfinite(up), (p - up.astype(LD)) / (1 + np.abs(np.where(np.isfinite(up), up, 0.0))), -np.inf)
    out["feas"] = float(max(0.0, below.max(), above.max()))
    out["dj"] = float(np.abs(d - (c[1:] - Al.T @ lam)).max())
    side, D = LD(0), c[0]
    for k in range(M + N):
        if abs(y[k]) <= DUAL_ZERO:
            bnd = lo[k] if y[k] > 0 else up[k]
            if np.isfinite(bnd):
                D += y[k] * LD(bnd)
            continue
        bnd = lo[k] if y[k] > 0 else up[k]
        if not np.isfinite(bnd):
            side = LD(np.inf)
            continue
        side = max(side, abs(p[k] - LD(bnd)))
        D += y[k] * LD(bnd)
    P = c[0] + c[1:] @ x
    out["side"] = float(side)
    out["gap"] = float(max(abs(D - P), abs(P - LD(z))))
    return out


def gap_bound(z, oracle_gap):
    """of the engine's duality gap: 1e-9 relative, or ten times what the oracle's own solutions of the shape leave (another pivot order)"""
    return max(RTOL * (1.0 + abs(z)), 10.0 * oracle_gap)


def assert_certified(res, z, oracle_gap, tag):
    assert res is not None, tag
    assert res["rows"] <= TOL_ROWS, (tag, res)
    assert res["feas"] <= TOL_FEAS, (tag, res)
    assert res["dj"] <= TOL_DJ, (tag, res)
    assert res["side"] <= TOL_SIDE, (tag, res)
    assert res["gap"] <= gap_bound(z, oracle_gap), (tag, res, gap_bound(z, oracle_gap))


def worst(rows):
    """the worst residual of each kind over some certificates"""
    rows = [r for r in rows if r is not None]
    return {k: max(r[k] for r in rows) for k in ("rows", "feas", "dj", "side", "gap")} if rows else None


# ---- the general sets ------------------------------------------------------------------------------------------------------
# (M, N) -> seed.  Chosen on the CPU (python tests/lp_cases.py): HiGHS and the oracle agree on every LP of both arrangements.
GENERAL_SEEDS = {(15, 16): 1, (16, 17): 2, (31, 64): 3, (32, 65): 4, (33, 257): 5, (24, 1120): 6, (24, 1121): 7, (24, 1535): 8,
                 (24, 1536): 9, (24, 2048): 10, (24, 2049): 11, (24, 4100): 12}
NLP = 16
BAD = 5                     # the LP that is infeasible by construction (inside the sub-batch of 7 as well)
PAIR_COLS = (2, 3, 5)       # the columns of the two rows with equal coefficients: boxed, inside the per-LP range of arrangement "b"
FAR = (10, 12, 14)
COL_FIRST = 1               # arrangement "b": the range starts at this (odd) column


def model_seed(M, N):
    """of general_model: GENERAL_SEEDS', or OBJECTIVE_SEEDS' (below) for the shapes that only the objective sets have"""
    return GENERAL_SEEDS[(M, N)] if (M, N) in GENERAL_SEEDS else OBJECTIVE_SEEDS[(M, N)]


def general_model(M, N):
    """the model of a shape: random_lp's feasible and bounded LP, with rows 0 and 1 made a pair with equal coefficients (row 0 bounded
    below, row 1 above) on three boxed columns and one column that starts on an artificial bound.  Returns a dict with A, cost, lo, up, x0 and the bound types of rows and columns."""
    rng = np.random.default_rng(model_seed(M, N))
    A, lo, up, cost, x0, tr, tc = random_lp(M, N, rng, "feasible", bounded=True, parts=True)
    cols = list(PAIR_COLS)
    A[0] = 0.0
    A[0, cols] = [1.0, -1.5, 2.0]
    # ... and on column N - 1, which has no other row, a lower bound only and a cost that pulls it up: dual infeasible in the standard
    # basis, so the engine gives it an artificial upper bound to start from; row 1 is what really holds it, and every LP stays bounded
    j = N - 1
    shift = -A[:, j] * x0[j]
    lo[:M], up[:M] = lo[:M] + shift, up[:M] + shift             # (the other rows stay around their value at x0)
    A[:, j] = 0.0
    A[0, j] = 1.0
    A[1] = A[0]
    tc[j], cost[1 + j] = "l", -2.0
    lo[M + j], up[M + j] = x0[j] - 1.0, np.inf
    tr[0], tr[1] = "l", "u"
    r = float(A[0] @ x0)
    lo[0], up[0], lo[1], up[1] = r - 1.0, np.inf, -np.inf, r + 1.0
    for j in cols:
        tc[j] = "d"
        lo[M + j], up[M + j] = x0[j] - 1.0, x0[j] + 2.0
    return dict(M=M, N=N, A=A, cost=cost, lo=lo, up=up, x0=x0, tr=tr, tc=tc, rng=rng)


def _typed(types, centre, rng, width):
    """bounds of the given types around `centre`: up to `width` below and above, 's' on it, 'd' with room"""
    n = len(types)
    l, u = centre - rng.integers(0, width + 1, size=n), centre + rng.integers(0, width + 1, size=n)
    l = np.where(types == "s", centre, l)
    u = np.where((types == "d") & (u == l), l + 1, u)
    return _bounds(types, l, u)


_SETS = {}


def general_set(M, N, arr):
    """One model and NLP LPs that differ only in the bounds of the per-LP range; every variable has the same finite and infinite
    sides in every LP and in the model (the contract of a DUAL start: the costs never change, a solved slot stays dual feasible).
      arr "a": var_first = 0, var_cnt = M: every row is per LP.  LP t has its rows around A x_t, x_t a point of the columns' box
               that lies further from x0 the larger t is; LP BAD asks row 0 >= v + 5 and row 1 <= v + 4.
      arr "b": var_cnt = min(N - 2, 40) columns from column 1, the rows shared.  LP t boxes the columns around x0, wider with t, and for
               t in FAR around points away from x0;
               LP BAD moves the boxes of the pair's columns so far that a.x >= a.x0 + 15 against row 1's a.x <= a.x0 + 1.
    LP 0 has the model's own bounds.  Returns a dict: the model, var_first, var_cnt, vlo / vup (NLP x var_cnt), perm (the second
    generation solves LP perm[b] from the slot of LP b) and lps, the full (lo, up) of every LP."""
    key = (M, N, arr)
    if key in _SETS:
        return _SETS[key]
    m = general_model(M, N)
    rng = np.random.default_rng(GENERAL_SEEDS[(M, N)] * 1000 + (1 if arr == "a" else 2))
    A, lo, up, x0, tr, tc = m["A"], m["lo"], m["up"], m["x0"], m["tr"], m["tc"]
    if arr == "a":
        first, cnt = 0, M
        types = tr
    else:
        first, cnt = M + COL_FIRST, min(N - 1 - COL_FIRST, 40)      # (column N - 1 stays the model's)
        types = tc[COL_FIRST:COL_FIRST + cnt]
    vlo, vup = np.tile(lo[first:first + cnt], (NLP, 1)), np.tile(up[first:first + cnt], (NLP, 1))
    clo, cup = lo[M:], up[M:]
    for t in range(1, NLP):
        if arr == "a":
            xt = np.clip(x0 + np.round(rng.normal(size=N) * 0.4 * t), clo, cup)      # (inside the columns' box: the LP is feasible)
            rt = A @ xt
            vlo[t], vup[t] = _typed(types, rt, rng, 2)
            if t == BAD:
                v = float(A[0] @ xt)
                vlo[t, 0], vup[t, 1] = v + 5.0, v + 4.0
        else:
            # (x0 stays inside: the LP is feasible.  Three LPs move their boxes away from x0 and the rows have to follow: what comes of
            # it is for the yardsticks to say, 12 LPs are OPTIMAL whatever they say)
            centre = x0[COL_FIRST:COL_FIRST + cnt] + (np.round(rng.normal(size=cnt) * t) if t in FAR else 0.0)
            vlo[t], vup[t] = _typed(types, centre, rng, 1 + t // 2)
            if t == BAD:
                for j in PAIR_COLS:
                    s = 1.0 if A[0, j] > 0 else -1.0
                    a, b = x0[j] + 10.0 * s, x0[j] + 11.0 * s
                    vlo[t, j - COL_FIRST], vup[t, j - COL_FIRST] = min(a, b), max(a, b)
    assert np.array_equal(np.isfinite(vlo), np.tile(np.isfinite(lo[first:first + cnt]), (NLP, 1)))
    assert np.array_equal(np.isfinite(vup), np.tile(np.isfinite(up[first:first + cnt]), (NLP, 1)))
    lps = []
    for t in range(NLP):
        l, u = lo.copy(), up.copy()
        l[first:first + cnt], u[first:first + cnt] = vlo[t], vup[t]
        lps.append((l, u))
    perm = (np.arange(NLP) * 7 + 3) % NLP         # a permutation without a fixed point among 16
    out = dict(m, arr=arr, var_first=first, var_cnt=cnt, vlo=vlo, vup=vup, lps=lps, perm=perm)
    _SETS[key] = out
    return out


def unbounded_model(M, N):
    """the model of the shape with column 0 taken out of every row, free and with a cost: (A, lo, up, cost)"""
    m = general_model(M, N)
    A, lo, up, cost = m["A"].copy(), m["lo"].copy(), m["up"].copy(), m["cost"].copy()
    A[:, 0] = 0.0
    lo[M], up[M], cost[1] = -np.inf, np.inf, 1.0
    return A, lo, up, cost


_REF = {}


def general_references(M, N, arr):
    """the LPs of a set with the answers of both yardsticks and the oracle's own certificate, computed once and shared:
    rows of dict(st, obj, st_highs, obj_highs, cert), and the oracle's worst residuals over the set"""
    key = (M, N, arr)
    if key not in _REF:
        s = general_set(M, N, arr)
        rows = []
        for lo, up in s["lps"]:
            so, zo, po, do = oracle_solution(s["A"], lo, up, s["cost"])
            sh, zh = highs(s["A"], lo, up, s["cost"])
            rows.append(dict(st=so, obj=zo, st_highs=sh, obj_highs=zh, cert=certify(s["A"], lo, up, s["cost"], so, zo, po, do)))
        _REF[key] = (rows, worst([r["cert"] for r in rows]))
    return _REF[key]


def assert_references_agree(M, N, arr):
    """what the tests assert of the yardsticks before they look at the engine"""
    rows, w = general_references(M, N, arr)
    for t, r in enumerate(rows):
        assert r["st"] == r["st_highs"], (M, N, arr, t, r["st"], r["st_highs"])
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(r["obj"], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg=str((M, N, arr, t)))
            assert_certified(r["cert"], r["obj"], r["cert"]["gap"], ("oracle", M, N, arr, t))
    assert rows[BAD]["st"] == INFEASIBLE, (M, N, arr, rows[BAD]["st"])
    assert sum(r["st"] == OPTIMAL for r in rows) >= 12, (M, N, arr, [r["st"] for r in rows])
    return rows, w


# ---- the objective sets ----------------------------------------------------------------------------------------------------
# Shapes that only the objective sets have, (M, N) -> seed of general_model.  Chosen on the CPU (python tests/lp_cases.py obj): both
# yardsticks call all 48 LPs of every set OPTIMAL and agree, and the conditions of assert_objective_references_agree hold.
OBJECTIVE_SEEDS = {(24, 512): 13, (24, 513): 14, (24, 1024): 15, (24, 1025): 16, (24, 8192): 17, (24, 8193): 18}
OBJ_SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 512), (24, 513), (24, 1024), (24, 1025), (24, 1120), (24, 1121),
              (24, 1535), (24, 1536), (24, 2048), (24, 2049), (24, 4100), (24, 8192), (24, 8193)]
OBJ_RANGES = ("cols", "straddle", "head")
GENS = ("gen1", "gen2", "gen3")
UNB_LPS = {2: 1.0, 9: 1.0, 5: -1.0}         # unbounded_objective_set: LP -> the cost of the free column without a row


def obj_ranges(M, N):
    """the cost ranges a shape runs: a slot of the two largest shapes is 2 MB, they run "cols" only"""
    return ("cols",) if N >= 8192 else OBJ_RANGES


def cost_range(M, N, rng_name):
    """(cost_first, cost_cnt) in the engine's numbering: rows 0 .. M-1, columns M .. M+N-1"""
    return {"cols": (M, N), "straddle": (M - 3, 8), "head": (M + 1, 5)}[rng_name]


def _signed(c, lo, up):
    """costs that pull no variable where it has no bound: f -> 0, l -> |c|, u -> -|c|, d and s as drawn"""
    flo, fup = np.isfinite(lo), np.isfinite(up)
    return np.where(flo & fup, c, np.where(flo, np.abs(c), np.where(fup, -np.abs(c), 0.0)))


def fold(A, first, c):
    """the cost vector (N + 1, no shift) of the columns alone that is the same function on r = A x as the costs c on the variables
    first .. first + len(c) - 1: c'_cols = c_cols + A' c_rows"""
    M, N = A.shape
    full = np.zeros(M + N)
    full[first:first + len(c)] = c
    return np.concatenate([[0.0], full[M:] + A.T @ full[:M]])


_OSETS = {}


def objective_set(M, N, rng_name):
    """The model of general_model(M, N) with a zero engine cost and NLP cost vectors over one range of variables in each of three
    generations: gen1 rounded normal values times 3, signed by the bound type of the variable that carries them (row or column), every
    fourth vector with 70 % of its entries zeroed (ties, and variables of the range without a cost); gen2 is gen1 permuted by `perm`
    (LP b of gen2 has the costs of LP perm[b] of gen1) times uniform(0.9, 1.1) entrywise; gen3 is gen2 times uniform(0.95, 1.05).
    Returns a dict: the model, cost_first, cost_cnt, costs (gen -> NLP x cost_cnt), folded (gen -> the NLP folded cost vectors the
    yardsticks and the certificate take) and perm."""
    key = (M, N, rng_name)
    if key in _OSETS:
        return _OSETS[key]
    m = general_model(M, N)
    A, lo, up = m["A"], m["lo"], m["up"]
    first, cnt = cost_range(M, N, rng_name)
    assert 0 <= first and first + cnt <= M + N
    rng = np.random.default_rng(model_seed(M, N) * 1000 + 10 + OBJ_RANGES.index(rng_name))
    vl, vu = lo[first:first + cnt], up[first:first + cnt]
    c1 = _signed(np.round(rng.normal(size=(NLP, cnt)) * 3), vl, vu)
    for t in range(3, NLP, 4):
        c1[t, rng.random(cnt) < 0.7] = 0.0
    perm = (np.arange(NLP) * 7 + 3) % NLP         # (general_set's)
    c2 = c1[perm] * rng.uniform(0.9, 1.1, size=(NLP, cnt))
    c3 = c2 * rng.uniform(0.95, 1.05, size=(NLP, cnt))
    costs = dict(gen1=c1, gen2=c2, gen3=c3)
    for c in costs.values():
        assert np.array_equal(c, _signed(c, vl, vu))
    folded = {g: [fold(A, first, c) for c in costs[g]] for g in GENS}
    out = dict(m, cost=np.zeros(N + 1), rng_name=rng_name, cost_first=first, cost_cnt=cnt, costs=costs, folded=folded, perm=perm)
    _OSETS[key] = out
    return out


def unbounded_objective_set(M, N):
    """unbounded_model(M, N) -- column 0 in no row and free -- with a zero engine cost and NLP cost vectors over the columns 0, 1, 2:
    (+1, 0, 0) or (-1, 0, 0) for the LPs of UNB_LPS, which are UNBOUNDED, and (0, c1, c2), signed by type, for the others"""
    A, lo, up, _ = unbounded_model(M, N)
    first, cnt = M, 3
    rng = np.random.default_rng(model_seed(M, N) * 1000 + 20)
    c = _signed(np.round(rng.normal(size=(NLP, cnt)) * 3), lo[first:first + cnt], up[first:first + cnt])
    c[:, 0] = 0.0
    for t, v in UNB_LPS.items():
        c[t] = (v, 0.0, 0.0)
    return dict(M=M, N=N, A=A, lo=lo, up=up, cost=np.zeros(N + 1), cost_first=first, cost_cnt=cnt, costs=c, folded=[fold(A, first, v) for v in c])


def _reference_rows(A, lo, up, folded):
    rows = []
    for c in folded:
        so, zo, po, do = oracle_solution(A, lo, up, c)
        sh, zh = highs(A, lo, up, c)
        rows.append(dict(st=so, obj=zo, st_highs=sh, obj_highs=zh, prim=po, dual=do, cert=certify(A, lo, up, c, so, zo, po, do)))
    return rows


_OREF = {}


def objective_references(M, N, rng_name):
    """the 3 x NLP LPs of an objective set with the answers of both yardsticks (for the folded costs), the oracle's solution and its own
    certificate, computed once and shared: gen -> rows of dict(st, obj, st_highs, obj_highs, prim, dual, cert), and the oracle's worst
    residuals over the set"""
    key = (M, N, rng_name)
    if key not in _OREF:
        s = objective_set(M, N, rng_name)
        ref = {g: _reference_rows(s["A"], s["lo"], s["up"], s["folded"][g]) for g in GENS}
        _OREF[key] = (ref, worst([r["cert"] for g in GENS for r in ref[g]]))
    return _OREF[key]


def _assert_rows_agree(rows, tag):
    for t, r in enumerate(rows):
        assert r["st"] == r["st_highs"], (tag, t, r["st"], r["st_highs"])
        if r["st"] == OPTIMAL:
            np.testing.assert_allclose(r["obj"], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg=str((tag, t)))
            assert_certified(r["cert"], r["obj"], r["cert"]["gap"], ("oracle", tag, t))


def assert_objective_references_agree(M, N, rng_name):
    """what the tests assert of the yardsticks, and of the inputs, before they look at the engine: all 48 LPs OPTIMAL for both, equal
    values, the oracle's solutions certified; in the union of the optimal points some boxed column on its upper and some on its lower
    bound, each with a non-zero reduced cost (places for bound flips); "cols": at least a quarter of the columns that carry a cost are
    nonbasic (a non-zero reduced cost, or more cost-carrying columns than the M a basis holds).  Returns (references, worst residuals, a dict of these counts)."""
    ref, w = objective_references(M, N, rng_name)
    s = objective_set(M, N, rng_name)
    lo, up = s["lo"][M:], s["up"][M:]
    boxed = np.isfinite(lo) & np.isfinite(up) & (lo < up)
    at_up = at_lo = 0
    carrying = nonbasic = 0
    for g in GENS:
        _assert_rows_agree(ref[g], (M, N, rng_name, g))
        for t, r in enumerate(ref[g]):
            assert r["st"] == OPTIMAL, (M, N, rng_name, g, t, r["st"])
            x, d = r["prim"][M:], r["dual"][M:]
            at_up += int(np.sum(boxed & (d < -DUAL_ZERO) & (np.abs(x - up) <= TOL_SIDE)))
            at_lo += int(np.sum(boxed & (d > DUAL_ZERO) & (np.abs(x - lo) <= TOL_SIDE)))
            if rng_name == "cols":
                c = s["costs"][g][t] != 0.0
                carrying += int(c.sum())
                nonbasic += max(int(np.sum(c & (np.abs(d) > DUAL_ZERO))), int(c.sum()) - M)
    assert at_up > 0 and at_lo > 0, (M, N, rng_name, at_up, at_lo)
    if rng_name == "cols":
        assert 4 * nonbasic >= carrying, (M, N, rng_name, nonbasic, carrying)
    return ref, w, dict(boxed_at_up=at_up, boxed_at_lo=at_lo, carrying=carrying, nonbasic=nonbasic)


_UREF = {}


def unbounded_objective_references(M, N):
    """rows as objective_references' for unbounded_objective_set, asserted: the LPs of UNB_LPS UNBOUNDED, the others OPTIMAL, for both
    yardsticks; and the oracle's worst residuals over the OPTIMAL ones"""
    if (M, N) not in _UREF:
        s = unbounded_objective_set(M, N)
        rows = _reference_rows(s["A"], s["lo"], s["up"], s["folded"])
        _assert_rows_agree(rows, (M, N, "unbounded"))
        for t, r in enumerate(rows):
            assert r["st"] == (UNBOUNDED if t in UNB_LPS else OPTIMAL), (M, N, t, r["st"])
        _UREF[(M, N)] = (rows, worst([r["cert"] for r in rows]))
    return _UREF[(M, N)]


def _main_obj(shapes):
    for M, N in shapes:
        for rng_name in obj_ranges(M, N):
            ref, w, n = assert_objective_references_agree(M, N, rng_name)
            print("lp_obj_general_residuals oracle M %d N %d range %s statuses %s boxed at up %d at lo %d%s rows %.3e feas %.3e dj %.3e side %.3e gap %.3e" % (
                M, N, rng_name, " ".join("".join(str(r["st"]) for r in ref[g]) for g in GENS), n["boxed_at_up"], n["boxed_at_lo"],
                " nonbasic %d of %d" % (n["nonbasic"], n["carrying"]) if rng_name == "cols" else "", w["rows"], w["feas"], w["dj"], w["side"], w["gap"]), flush=True)
        if N < 8192:
            rows, w = unbounded_objective_references(M, N)
            print("lp_obj_general_residuals oracle M %d N %d unbounded objectives statuses %s gap %.3e" % (M, N, "".join(str(r["st"]) for r in rows), w["gap"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "obj":
        v = [int(a) for a in sys.argv[2:]]
        _main_obj(list(zip(v[0::2], v[1::2])) if v else OBJ_SHAPES)
        sys.exit(0)
    shapes = list(GENERAL_SEEDS)
    if len(sys.argv) > 1:
        v = [int(a) for a in sys.argv[1:]]
        shapes = list(zip(v[0::2], v[1::2]))
    for M, N in shapes:
        for arr in ("a", "b"):
            rows, w = assert_references_agree(M, N, arr)
            print("lp_general_residuals oracle M %d N %d arr %s statuses %s rows %.3e feas %.3e dj %.3e side %.3e gap %.3e" % (
                M, N, arr, "".join(str(r["st"]) for r in rows), w["rows"], w["feas"], w["dj"], w["side"], w["gap"]), flush=True)
        A, lo, up, cost = unbounded_model(M, N)
        so, sh = oracle_primal(A, lo, up, cost)[0], highs(A, lo, up, cost)[0]
        assert so == sh == UNBOUNDED, (M, N, so, sh)
        print("lp_general_residuals unbounded model M %d N %d: oracle %d HiGHS %d" % (M, N, so, sh), flush=True)
