"""GPU: bslv_lpq_certify, the optimality certificate of solved slots computed on the device (bensolve_amd/csrc/lp_certify.inc), against
its yardstick: tests/lp_cases.py: certify in np.longdouble on the vectors the GETTERS return for the same slots.  Never against a
second run of the code under test.

The bound of every comparison (derived, not measured): |device - host| <= 2^-52 |host| + 2 (L + 2) eps_LD S, with eps_LD the epsilon
of np.longdouble, L the number of terms of the longest sum of the kind and S the largest sum of |terms| of the kind, both computed here
in numpy for the LP at hand (_terms).  The first term is the device's one final rounding (its sums are compensated: as if formed in
twice the working precision), the second the host's longdouble summation error, doubled to cover the device's second-order term.
rows: r_i and the N products of row i; dj: d_j, c_j and the M products of column j; feas and side: the value and its bound; gap: the
terms of P, of D, and z.  side = inf has to agree as inf.  Where np.longdouble is no wider than double the comparison is skipped.

Shapes of the kernel's own edges (test 3; constants of lp_certify.inc).  The dense products of the tableau form stage tiles of
CERT_TK = 32 terms x CERT_TO = 64 outputs; A x has M outputs and N terms, A' lambda has N outputs and M terms:
  (31, 63) (32, 64) (33, 65)   M one below, at, one above CERT_TK (terms of A' lambda) and N the same around CERT_TO (its outputs);
  (63, 31) (64, 32) (65, 33)   M around CERT_TO (outputs of A x), N around CERT_TK (its terms)
The compressed products of the revised form take CERT_SR = 16 lines per workgroup and stage CERT_G = 16 entries of a line at a time:
  (15, 26) (16, 27) (17, 28)   M around CERT_SR (lines of the CSR); the rows hold about 0.6 N entries: 8 .. 18, 11 .. 16 and 10 .. 19 of them,
                               so lines shorter than, of exactly and longer than CERT_G occur (asserted); the columns hold 4 .. 13
Every shape with B = 1, 15, 16, 17, 33 LPs: one below, at, one above the group of CERT_G = 16 LPs, and two groups and one.
Objective batches (test 4) take generation 1 of lp_cases.objective_set: its costs are integers and A holds multiples of 1/2, so
lp_cases.fold's column cost is exact in double and the yardstick sees the very cost vector the device certifies."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lp_cases as lc
from lp_cases import OPTIMAL, NLP, DUAL_ZERO
from test_lp_general_gpu import _env, _engine, _solve

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
KINDS = ("rows", "feas", "dj", "side", "gap")
G = 16
NONE = np.zeros((1, 0))
E_ARG = 2


def _terms(A, lo, up, cost, z, prim, dual):
    """kind -> (L, S) of one LP: the terms of the longest sum and the largest sum of |terms| (see the module's docstring)"""
    M, N = A.shape
    x, r, lam, d = prim[M:], prim[:M], dual[:M], dual[M:]
    absA = np.abs(A)
    out = {}
    out["rows"] = (N + 1, float((np.abs(r) + absA @ np.abs(x)).max()))
    out["dj"] = (M + 2, float((np.abs(d) + np.abs(cost[1:]) + absA.T @ np.abs(lam)).max()))
    flo, fup = np.isfinite(lo), np.isfinite(up)
    s = [0.0]
    if flo.any():
        s.append(float((np.abs(lo[flo]) + np.abs(prim[flo])).max()))
    if fup.any():
        s.append(float((np.abs(up[fup]) + np.abs(prim[fup])).max()))
    out["feas"] = (2, max(s) + 1.0)
    bnd = np.where(dual > 0, lo, up)
    fin = np.isfinite(bnd)
    nz = (np.abs(dual) > DUAL_ZERO) & fin
    out["side"] = (2, float((np.abs(prim[nz]) + np.abs(bnd[nz])).max()) if nz.any() else 0.0)
    sp = abs(cost[0]) + float(np.abs(cost[1:] * x).sum())
    sd = abs(cost[0]) + float(np.abs(dual[fin] * bnd[fin]).sum())
    out["gap"] = ((N + 1) + (M + N + 1) + 1, sp + sd + abs(z))
    return out


def _assert_close(dev, host, terms, tag):
    """the five values of one LP against the yardstick's, each within its derived bound; prints the figures before it asserts"""
    if EPS_LD >= float(np.finfo(np.float64).eps):
        pytest.skip("np.longdouble is no wider than double here: the yardstick is no more accurate than the device")
    for k, name in enumerate(KINDS):
        d, h = float(dev[k]), float(host[name])
        if np.isinf(h):
            assert np.isinf(d) and d > 0, (tag, name, d, h)
            continue
        L, S = terms[name]
        bound = 2.0 ** -52 * abs(h) + 2.0 * (L + 2) * EPS_LD * S
        if abs(d - h) > bound:
            print("certify mismatch %s %s: device %.17e host %.17e diff %.3e bound %.3e (L %d S %.3e)" % (tag, name, d, h, abs(d - h), bound, L, S))
        assert abs(d - h) <= bound, (tag, name, d, h, abs(d - h), bound)


def _compare(eng, A, cost_of, bounds_of, slots, out, tag, check_at=True):
    """the device's answer `out` for `slots` against lp_cases.certify on the getters' vectors; cost_of(b) / bounds_of(b): the full cost
    vector (N + 1) and the full (lo, up) of LP b.  Returns the yardstick's certificates."""
    M, N = A.shape
    n = M + N
    prim, dual, obj = eng.primal(slots, 0, n), eng.dual(slots, 0, n), eng.obj(slots)
    certs = []
    for b in range(len(slots)):
        lo, up = bounds_of(b)
        cost = cost_of(b)
        host = lc.certify(A, lo, up, cost, OPTIMAL, obj[b], prim[b], dual[b])
        terms = _terms(A, lo, up, cost, obj[b], prim[b], dual[b])
        _assert_close(out["res"][b], host, terms, tag + (b,))
        certs.append(host)
        at = out["at"][b]
        assert at[4] == -1, (tag, b, at)
        if check_at:
            assert 0 <= at[0] < M and M <= at[2] < n and -1 <= at[1] < n and -1 <= at[3] < n, (tag, b, at)
            # the residual at the variable the device names is the worst one (within the bound of the kind)
            Al, p, y = A.astype(LD), prim[b].astype(LD), dual[b].astype(LD)
            rr = np.abs(p[:M] - Al @ p[M:])
            dd = np.abs(y[M:] - (np.asarray(cost, LD)[1:] - Al.T @ y[:M]))
            for val, worst, name in ((rr[at[0]], rr.max(), "rows"), (dd[at[2] - M], dd.max(), "dj")):
                L, S = terms[name]
                assert abs(float(val) - float(worst)) <= 2.0 ** -52 * abs(float(worst)) + 4.0 * (L + 2) * EPS_LD * S, (tag, b, name, at, float(val), float(worst))
            if at[3] >= 0:
                assert abs(dual[b][at[3]]) > DUAL_ZERO, (tag, b, at)
            else:
                assert not np.any(np.abs(dual[b]) > DUAL_ZERO), (tag, b, at)
    return certs


def _certified(cert, z, oracle_gap):
    try:
        lc.assert_certified(cert, z, oracle_gap, "")
        return True
    except AssertionError:
        return False


# ---- 1. / 2. agreement with the yardstick on the general sets, both forms ------------------------------------------------------
def _general(M, N, arr, form):
    s = lc.general_set(M, N, arr)
    _, oracle = lc.assert_references_agree(M, N, arr)
    vlo, vup = s["vlo"], s["vup"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], 1 + NLP, form)
    try:
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
        assert st[0] == OPTIMAL
        dst = np.arange(1, 1 + NLP, dtype=np.int32)
        st, _, _ = _solve(eng, np.zeros(NLP, np.int32), dst, vlo, vup, retry)
        opt = np.nonzero(st == OPTIMAL)[0]
        assert len(opt) >= 12, (M, N, arr, form, st)
        out = eng.certify(dst[opt], vlo[opt], vup[opt])          # ONE call for all of them
        stats = eng.last_certify_stats()
        assert stats["lps"] == len(opt) and stats["launches"] >= 4, stats
        tag = (form, M, N, arr)
        certs = _compare(eng, s["A"], lambda b: s["cost"], lambda b: s["lps"][opt[b]], dst[opt], out, tag)
        obj = eng.obj(dst[opt])
        for b, c in enumerate(certs):
            if _certified(c, obj[b], oracle["gap"]):
                assert out["verdict"][b] == 0, (tag, b, out["verdict"][b], out["res"][b], c)
        assert stats["not_certified"] == int(np.sum(out["verdict"] != 0))
        w = out["res"].max(axis=0)
        print("lp_certify device %s M %d N %d arr %s lps %d rows %.3e feas %.3e dj %.3e side %.3e gap %.3e" % (form, M, N, arr, len(opt), *w))
    finally:
        eng.close()


@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 1121)])
def test_agrees_with_the_yardstick_tableau_form(oracle, M, N, arr):
    _general(M, N, arr, "tableau")


@pytest.mark.parametrize("M,N", [(33, 257), (24, 2049), (24, 4100)])
def test_agrees_with_the_yardstick_revised_form(oracle, M, N):
    _general(M, N, "a", "revised")


# ---- 3. the kernel's own edges ----------------------------------------------------------------------------------------------
BATCHES = (1, G - 1, G, G + 1, 2 * G + 1)
NB = max(BATCHES)


def _edge_case(M, N, seed):
    """a feasible and bounded random model, the rows per LP: LP t has the model's row bounds widened by (t % 4) / 2 (LP 0: the model's)"""
    rng = np.random.default_rng(seed)
    A, lo, up, cost = lc.random_lp(M, N, rng, "feasible", bounded=True)
    w = 0.5 * (np.arange(NB) % 4)[:, None]
    vlo, vup = lo[None, :M] - w, up[None, :M] + w          # (an infinite bound stays infinite)
    lps = []
    for t in range(NB):
        l, u = lo.copy(), up.copy()
        l[:M], u[:M] = vlo[t], vup[t]
        lps.append((l, u))
    return A, lo, up, cost, np.ascontiguousarray(vlo), np.ascontiguousarray(vup), lps


def _edges(M, N, form):
    A, lo, up, cost, vlo, vup, lps = _edge_case(M, N, 100 * M + N)
    if form == "revised":
        rl, cl = (A != 0).sum(axis=1), (A != 0).sum(axis=0)
        assert rl.min() < G <= rl.max(), rl
        assert cl.min() < G, cl
    retry = form == "revised"
    eng = _engine(A, lo, up, cost, 0, M, 1 + NB, form)
    try:
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
        assert st[0] == OPTIMAL, st
        dst = np.arange(1, 1 + NB, dtype=np.int32)
        st, _, _ = _solve(eng, np.zeros(NB, np.int32), dst, vlo, vup, retry)
        assert np.all(st == OPTIMAL), (M, N, form, st)          # (feasible and bounded by construction)
        for B in BATCHES:
            out = eng.certify(dst[:B], vlo[:B], vup[:B])
            assert eng.last_certify_stats()["lps"] == B
            _compare(eng, A, lambda b: cost, lambda b: lps[b], dst[:B], out, (form, M, N, "B", B))
    finally:
        eng.close()


@pytest.mark.parametrize("M,N", [(31, 63), (32, 64), (33, 65), (63, 31), (64, 32), (65, 33)])
def test_tile_edges_of_the_dense_products(M, N):
    _edges(M, N, "tableau")


@pytest.mark.parametrize("M,N", [(15, 26), (16, 27), (17, 28)])
def test_tile_edges_of_the_compressed_products(M, N):
    _edges(M, N, "revised")


# ---- 4. objective batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("rng_name", lc.OBJ_RANGES)
@pytest.mark.parametrize("M,N", [(16, 17), (33, 257)])
def test_objective_batches(oracle, M, N, rng_name, form):
    from test_lp_obj_general_gpu import _feasible_start, _solve_obj
    s = lc.objective_set(M, N, rng_name)
    first, C = s["cost_first"], s["costs"]["gen1"]
    for c, f in zip(C, s["folded"]["gen1"]):          # (generation 1: the folded cost is exact, see the module's docstring)
        full = np.zeros(M + N)
        full[first:first + len(c)] = c
        assert np.array_equal(f[1:].astype(LD), full[M:].astype(LD) + s["A"].T.astype(LD) @ full[:M].astype(LD))
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, 1 + NLP, form)
    try:
        _feasible_start(eng, 0, NONE, NONE)
        dst = np.arange(1, 1 + NLP, dtype=np.int32)
        st, _, _ = _solve_obj(eng, np.zeros(NLP, np.int32), dst, first, C, form == "revised")
        opt = np.nonzero(st == OPTIMAL)[0]
        assert len(opt) >= 12, (M, N, rng_name, form, st)
        out = eng.certify(dst[opt], cost_first=first, costs=C[opt])
        folded = s["folded"]["gen1"]
        _compare(eng, s["A"], lambda b: folded[opt[b]], lambda b: (s["lo"], s["up"]), dst[opt], out, (form, M, N, rng_name))
        # the engine's own (zero) cost is another LP: the same slots are not certified for it unless their duals vanish
        own = eng.certify(dst[opt])
        _compare(eng, s["A"], lambda b: s["cost"], lambda b: (s["lo"], s["up"]), dst[opt], own, (form, M, N, rng_name, "own cost"))
    finally:
        eng.close()


# ---- 5. folded rows --------------------------------------------------------------------------------------------------------------
def _folded_case():
    """random_lp(12, 20) with the rows per LP and three more rows of a single non-zero each outside that range: a lower bound on column 3
    that is tighter than the column's own and that its cost pushes it against, an upper bound on column 5 with a negative coefficient,
    and a range on column 7"""
    M, N = 12, 20
    rng = np.random.default_rng(4242)
    A, lo, up, cost, x0, tr, tc = lc.random_lp(M, N, rng, "feasible", bounded=True, parts=True)
    extra = np.zeros((3, N))
    extra[0, 3], extra[1, 5], extra[2, 7] = 2.0, -1.5, 0.5
    A2 = np.vstack([A, extra])
    rlo = np.concatenate([lo[:M], [2.0 * x0[3] - 1.0, -np.inf, 0.5 * x0[7] - 0.25]])
    rup = np.concatenate([up[:M], [np.inf, -1.5 * x0[5] + 0.75, 0.5 * x0[7] + 0.5]])
    clo, cup = lo[M:].copy(), up[M:].copy()
    clo[3], cup[3] = x0[3] - 5.0, x0[3] + 5.0
    cost = cost.copy()
    cost[1 + 3] = 3.0
    return A2, np.concatenate([rlo, clo]), np.concatenate([rup, cup]), cost, M


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_folded_rows_are_certified_in_the_indices_of_the_model_as_given(form):
    A, lo, up, cost, Mr = _folded_case()
    M, N = A.shape
    B = 5
    w = 0.5 * np.arange(B)[:, None]
    vlo, vup = np.ascontiguousarray(lo[None, :Mr] - w), np.ascontiguousarray(up[None, :Mr] + w)
    lps = []
    for t in range(B):
        l, u = lo.copy(), up.copy()
        l[:Mr], u[:Mr] = vlo[t], vup[t]
        lps.append((l, u))
    eng = _engine(A, lo, up, cost, 0, Mr, 1 + B, form)
    try:
        assert eng.rows_folded() >= 1
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], form == "revised")
        assert st[0] == OPTIMAL
        dst = np.arange(1, 1 + B, dtype=np.int32)
        st, _, _ = _solve(eng, np.zeros(B, np.int32), dst, vlo, vup, form == "revised")
        assert np.all(st == OPTIMAL), st
        out = eng.certify(dst, vlo, vup)
        certs = _compare(eng, A, lambda b: cost, lambda b: lps[b], dst, out, (form, "folded"))
        dual = eng.dual(dst, 0, M + N)
        print("folded rows: %d, duals of the folded rows %s, device residuals %s" % (eng.rows_folded(), dual[:, Mr:M].tolist(), out["res"].max(axis=0)))
        assert np.all(out["verdict"] == 0), (out["verdict"], out["res"], certs)
        assert eng.debug_poke(int(dst[0]), 0, 0, 1e-6) == E_ARG
    finally:
        eng.close()


# ---- 6. detection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_detects_what_is_poked(oracle, form):
    M, N = 16, 17
    s = lc.general_set(M, N, "a")          # (the rows are the per-LP range)
    A, cost = s["A"], s["cost"]
    retry = form == "revised"
    eng = _engine(A, s["lo"], s["up"], cost, s["var_first"], s["var_cnt"], 8, form)
    try:
        assert eng.rows_folded() == 0
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], s["vlo"][:1], s["vup"][:1], retry)
        assert st[0] == OPTIMAL
        # an LP of the set whose solution has a basic row strictly inside its bounds, a nonbasic column and a row with a non-zero dual;
        # it is solved five times from the parent, one slot per poke
        dst = np.arange(1, 6, dtype=np.int32)
        pick = None
        for t in range(NLP):
            if t == lc.BAD:
                continue
            one = slice(t, t + 1)
            vlo, vup = s["vlo"][one], s["vup"][one]
            st, _, _ = _solve(eng, np.zeros(5, np.int32), dst, np.repeat(vlo, 5, 0), np.repeat(vup, 5, 0), retry)
            if not np.all(st == OPTIMAL):
                continue
            P, Y = eng.primal(dst, 0, M + N), eng.dual(dst, 0, M + N)
            assert all(np.array_equal(P[0], P[k]) and np.array_equal(Y[0], Y[k]) for k in range(5))
            p, y = P[0], Y[0]
            lo, up = s["lps"][t]
            inside = [i for i in range(M) if y[i] == 0.0 and (np.isfinite(lo[i]) or np.isfinite(up[i])) and lo[i] + 1e-3 < p[i] < up[i] - 1e-3]
            nbcol = [j for j in range(N) if abs(y[M + j]) > 1e-6]
            drow = [i for i in range(M) if abs(y[i]) > 1e-6 and np.isfinite(lo[i] if y[i] > 0 else up[i])]
            flow = [i for i in range(M) if np.isfinite(lo[i])]
            if inside and nbcol and drow and flow:
                pick = (t, inside[0], nbcol[0], drow[0], flow[0])
                break
        assert pick is not None
        t, irow, jcol, idual, ilow = pick
        bounds = lambda b: s["lps"][t]
        base = eng.certify(dst[:1], vlo, vup)
        _compare(eng, A, lambda b: cost, bounds, dst[:1], base, (form, "base"))
        assert base["verdict"][0] == 0, base
        # a basic row variable's value
        assert eng.debug_poke(int(dst[1]), 0, irow, 1e-6) == 0
        out = eng.certify(dst[1:2], vlo, vup)
        _compare(eng, A, lambda b: cost, bounds, dst[1:2], out, (form, "value"))
        assert out["res"][0, 0] >= 5e-7 and out["verdict"][0] & 1 and out["at"][0, 0] == irow, (out, irow)
        # a nonbasic column's reduced cost
        assert eng.debug_poke(int(dst[2]), 1, M + jcol, 1e-5) == 0
        out = eng.certify(dst[2:3], vlo, vup)
        _compare(eng, A, lambda b: cost, bounds, dst[2:3], out, (form, "reduced cost"))
        assert out["res"][0, 2] >= 5e-6 and out["verdict"][0] & 4 and out["at"][0, 2] == M + jcol, (out, jcol)
        assert eng.debug_poke(int(dst[2]), 1, irow, 1e-5) == E_ARG          # (a basic variable has no stored reduced cost)
        # a per-LP bound moved past the returned value
        p = eng.primal(dst[3:4], 0, M + N)[0]
        wrong = vlo.copy()
        wrong[0, ilow] = p[ilow] + 1e-3
        lo2, up2 = s["lps"][t][0].copy(), s["lps"][t][1]
        lo2[ilow] = wrong[0, ilow]
        out = eng.certify(dst[3:4], wrong, vup)
        _compare(eng, A, lambda b: cost, lambda b: (lo2, up2), dst[3:4], out, (form, "bound"))
        assert out["res"][0, 1] > 0 and out["verdict"][0] & 2, out
        # a slot named twice, with the right and the wrong bounds: both answers in one call
        two = eng.certify([dst[3], dst[3]], np.vstack([vlo, wrong]), np.vstack([vup, vup]))
        assert two["verdict"][0] == 0 and two["verdict"][1] & 2, two
        assert np.array_equal(two["res"][1].view(np.uint64), out["res"][0].view(np.uint64))
        # the bound of a variable with a non-zero dual moves: side moves by that amount
        y = eng.dual(dst[4:5], 0, M + N)[0]
        mv_lo, mv_up = vlo.copy(), vup.copy()
        lo3, up3 = s["lps"][t][0].copy(), s["lps"][t][1].copy()
        if y[idual] > 0:
            mv_lo[0, idual] -= 0.25
            lo3[idual] -= 0.25
        else:
            mv_up[0, idual] += 0.25
            up3[idual] += 0.25
        out = eng.certify(dst[4:5], mv_lo, mv_up)
        _compare(eng, A, lambda b: cost, lambda b: (lo3, up3), dst[4:5], out, (form, "side"))
        assert abs(out["res"][0, 3] - 0.25) <= base["res"][0, 3] + 1e-12 and out["verdict"][0] & 8 and out["at"][0, 3] == idual, (out, base)
        if form == "revised":
            # drift in the stored inverse of a parent, a child solved from it: the certificate of the child against the yardstick, whatever it says
            eng.debug_perturb_inverse(int(dst[0]), 1e-6)
            t2 = int(s["perm"][t])
            st, it = eng.solve_batch([dst[0]], [6], s["vlo"][t2:t2 + 1], s["vup"][t2:t2 + 1])
            print("drifted parent (B^-1 perturbed by 1e-6 relative): child status %d after %d pivots" % (st[0], it[0]))
            if st[0] == OPTIMAL:
                out = eng.certify([6], s["vlo"][t2:t2 + 1], s["vup"][t2:t2 + 1])
                _compare(eng, A, lambda b: cost, lambda b: s["lps"][t2], [6], out, (form, "drifted child"))
                print("drifted child: verdict %d rows %.3e feas %.3e dj %.3e side %.3e gap %.3e at %s" % (out["verdict"][0], *out["res"][0], out["at"][0].tolist()))
    finally:
        eng.close()


# ---- 7. read-only and deterministic ----------------------------------------------------------------------------------------------
def _bytes(out):
    return out["res"].tobytes() + out["at"].tobytes() + out["verdict"].tobytes()


def _sequence(M, N, form, certify):
    s = lc.general_set(M, N, "a")
    vlo, vup, perm = s["vlo"], s["vup"], s["perm"]
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], 1 + 2 * NLP, form)
    h = hashlib.sha256()
    try:
        g1, g2 = np.arange(1, 1 + NLP, dtype=np.int32), np.arange(1 + NLP, 1 + 2 * NLP, dtype=np.int32)
        eng.reset_slot(0)
        st, it = eng.solve_batch([0], [0], vlo[:1], vup[:1])
        h.update(st.tobytes() + it.tobytes())
        st, it = eng.solve_batch(np.zeros(NLP, np.int32), g1, vlo, vup)
        h.update(st.tobytes() + it.tobytes())
        if certify:
            opt = st == OPTIMAL
            a = eng.certify(g1[opt], vlo[opt], vup[opt])
            b = eng.certify(g1[opt], vlo[opt], vup[opt])
            assert _bytes(a) == _bytes(b)          # the same call on the same state: the same bits
            with _env(BSLV_LP_CERTIFY_CHUNK="5"):          # ... also when the call runs in chunks of 5 LPs
                c = eng.certify(g1[opt], vlo[opt], vup[opt])
            assert _bytes(a) == _bytes(c)
        st, it = eng.solve_batch(g1, g2, vlo[perm], vup[perm])
        h.update(st.tobytes() + it.tobytes())
        n = M + N
        for sl in ([0], g1, g2):
            h.update(eng.obj(sl).tobytes() + eng.primal(sl, 0, n).tobytes() + eng.dual(sl, 0, n).tobytes())
    finally:
        eng.close()
    return h.hexdigest()


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_read_only_and_deterministic(oracle, form):
    M, N = (32, 65) if form == "tableau" else (33, 257)
    assert _sequence(M, N, form, True) == _sequence(M, N, form, False)


def test_lazily_open_and_parked_slots_give_the_same_bytes(oracle):
    M, N = 32, 65
    s = lc.general_set(M, N, "a")
    vlo, vup = s["vlo"], s["vup"]
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], 1 + NLP, "tableau")
    try:
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [0], vlo[:1], vup[:1])
        assert st[0] == OPTIMAL
        eng.set_lazy(1)
        dst = np.arange(1, 1 + NLP, dtype=np.int32)
        st, it = eng.solve_batch(np.zeros(NLP, np.int32), dst, vlo, vup)
        before = eng.lazy_stats()["on_request"]
        opt = st == OPTIMAL
        a = eng.certify(dst[opt], vlo[opt], vup[opt])
        _compare(eng, s["A"], lambda b: s["cost"], lambda b: s["lps"][np.nonzero(opt)[0][b]], dst[opt], a, ("lazy", M, N))
        eng.park(dst[:8])
        b = eng.certify(dst[opt], vlo[opt], vup[opt])
        eng.materialise(dst)
        assert eng.lazy_stats()["on_request"] > before          # (some of the slots were without their tableau until now)
        c = eng.certify(dst[opt], vlo[opt], vup[opt])
        assert _bytes(a) == _bytes(b) == _bytes(c)
    finally:
        eng.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(oracle):
    import ctypes
    M, N = 15, 16
    s = lc.general_set(M, N, "a")
    vlo, vup = s["vlo"], s["vup"]
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], 4, "tableau")
    try:
        eng.reset_slot(0)
        st0, it0 = eng.solve_batch([0], [1], vlo[:1], vup[:1])
        assert st0[0] == OPTIMAL
        before = (eng.obj([1]).tobytes(), eng.primal([1], 0, M + N).tobytes(), eng.dual([1], 0, M + N).tobytes())
        lib, vp, i = eng.lib, ctypes.c_void_p, ctypes.c_int
        lib.bslv_lpq_certify.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp]
        res, at, vd = np.zeros((2, 5)), np.zeros((2, 5), np.int32), np.zeros(2, np.int32)
        lo1, up1 = np.ascontiguousarray(vlo[:2]), np.ascontiguousarray(vup[:2])
        costs = np.zeros((2, 4))

        def call(B, slots, lo=lo1, up=up1, first=0, cnt=0, c=None):
            sl = np.ascontiguousarray(slots, np.int32)
            return lib.bslv_lpq_certify(eng.h, B, sl.ctypes.data, None if lo is None else lo.ctypes.data, None if up is None else up.ctypes.data, first, cnt,
                                        None if c is None else c.ctypes.data, None, res.ctypes.data, at.ctypes.data, vd.ctypes.data)

        assert call(1, [4]) == E_ARG and call(1, [-1]) == E_ARG          # a slot out of range
        assert call(-1, [1]) == E_ARG                                     # B < 0
        assert call(1, [1], lo=None) == E_ARG and call(1, [1], up=None) == E_ARG          # var_cnt > 0 without bounds
        assert call(1, [1], first=M + N - 3, cnt=4, c=costs) == E_ARG and call(1, [1], first=-1, cnt=2, c=costs) == E_ARG          # a cost range outside the model
        assert call(1, [1], first=0, cnt=4, c=None) == E_ARG
        assert call(0, [1]) == 0                                          # nothing to do
        assert call(1, [1]) == 0 and vd[0] == 0, (res, vd)
        after = (eng.obj([1]).tobytes(), eng.primal([1], 0, M + N).tobytes(), eng.dual([1], 0, M + N).tobytes())
        assert before == after
        st1, it1 = eng.solve_batch([0], [2], vlo[:1], vup[:1])          # the engine solves as before
        assert st1[0] == st0[0] and it1[0] == it0[0]
        assert eng.obj([2]).tobytes() == before[0] and eng.primal([2], 0, M + N).tobytes() == before[1] and eng.dual([2], 0, M + N).tobytes() == before[2]
    finally:
        eng.close()
