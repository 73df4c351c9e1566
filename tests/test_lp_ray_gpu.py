"""GPU: the ray store of the LP engine (bslv_lpq_set_rays: k_ray in bensolve_amd/csrc/lp_engine.hip) and its certificate
(bslv_lpq_certify_rays: k_cert_ray_final in lp_certify.inc) against the yardstick tests/lp_ray_cases.py: certify_ray in np.longdouble ON
THE VECTOR bslv_lpq_get_ray RETURNED.  Never against a second run of the code under test.

The bound of every comparison of residuals is the rule of tests/test_lp_certify_gpu.py, derived and not measured:
|device - host| <= 2^-52 |host| + 2 (L + 2) eps_LD S, L the terms of the longest sum of the kind and S its largest sum of |terms|
(lp_ray_cases.ray_terms).  Where np.longdouble is no wider than double the comparison is skipped.

Shapes: the tile edges of CERT_TO = 64, CERT_TK = 32 and CERT_G = 16 and the kernel edges lp_cases.GENERAL_SEEDS names
(lp_ray_cases.SHAPES); the certificate is asked for B = 1, 16 and 17 slots (one slot named twice)."""
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
from lp_cases import OPTIMAL, INFEASIBLE, UNBOUNDED, NLP, BAD
from lp_ray_cases import NONE as K_NONE, FARKAS, DIRECTION, BAD_LPS
from test_lp_general_gpu import _env, _engine, _solve
from test_lp_obj_general_gpu import _feasible_start, _solve_obj

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
EMPTY = np.zeros((1, 0))
E_ARG, E_STATE = 2, 5
DUAL, PRIMAL = 0, 1
DANTZIG, DEVEX = 0, 1
CLI = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
EXDIR = os.path.join(ROOT, "tests", "golden", "ex")


def _ray_engine(A, lo, up, cost, first, cnt, slots, form, by_env=False):
    with _env(BSLV_LP_RAYS="1" if by_env else None):
        eng = _engine(A, lo, up, cost, first, cnt, slots, form)
    assert eng.get_rays() == int(by_env)
    if not by_env:
        assert eng.set_rays(1) == 0
    assert eng.get_rays() == 1
    return eng


def _agree(dev, at, verdict, host, terms, tag):
    """the device's residuals, open entry and verdict of one LP against the yardstick's on the same vector"""
    assert int(verdict) == host["verdict"], (tag, int(verdict), host, dev)
    if host["verdict"] & 8:
        assert np.isnan(dev).all() and (np.asarray(at) == -1).all(), (tag, dev, at)
        return
    assert int(at[1]) == int(host["at"][1]) and at[2] == -1 and at[3] == -1, (tag, at, host["at"])
    if EPS_LD >= float(np.finfo(np.float64).eps):
        return          # (np.longdouble is no wider than double here: the yardstick is no more accurate than the device)
    for k in range(4):
        d, h = float(dev[k]), float(host["res"][k])
        L, S = terms[k]
        bound = 2.0 ** -52 * abs(h) + 2.0 * (L + 2) * EPS_LD * S
        if not abs(d - h) <= bound:
            print("certify_rays mismatch %s res[%d]: device %.17e host %.17e diff %.3e bound %.3e (L %d S %.3e)" % (tag, k, d, h, abs(d - h), bound, L, S))
        assert abs(d - h) <= bound, (tag, k, d, h, abs(d - h), bound)


def _compare(eng, A, slots, bounds_of, cost_of, out, tag):
    """out (certify_rays of slots) against certify_ray on what get_ray returns; returns (kinds, rays, the yardstick's answers)"""
    kinds, rays = eng.get_ray(slots)
    host = []
    for b in range(len(slots)):
        lo, up = bounds_of(b)
        h = rc.certify_ray(A, lo, up, cost_of(b), int(kinds[b]), rays[b])
        t = rc.ray_terms(A, lo, up, cost_of(b), int(kinds[b]), rays[b]) if kinds[b] != K_NONE else None
        _agree(out["res"][b], out["at"][b], out["verdict"][b], h, t, tag + (b,))
        host.append(h)
    return kinds, rays, host


# ---- 1. the hand-made LP ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_hand_made_lp(form):
    A, lo, up, cost = rc.handmade()
    eng = _ray_engine(A, lo, up, cost, 0, 0, 2, form, by_env=True)
    try:
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [1], EMPTY, EMPTY, form == "revised")
        assert st[0] == INFEASIBLE, st
        assert eng.last_ray_stats() == dict(farkas=1, direction=0, none=0)
        kind, ray = eng.get_ray([1])
        assert kind[0] == FARKAS and np.array_equal(ray[0], [1.0, -1.0, -1.0]), (kind, ray)          # (-z needs the row's upper bound: no proof)
        out = eng.certify_rays([1])
        # S = 3 - 1 - 1 and sum |z bound| = 3 + 1 + 1 by the definition of res[3]
        assert list(out["res"][0]) == [0.0, 0.0, 1.0, 5.0] and out["verdict"][0] == 0 and list(out["at"][0][1:]) == [-1, -1, -1], out
        assert eng.last_ray_certify_stats()["lps"] == 1 and eng.last_ray_certify_stats()["not_certified"] == 0
        # the slot that was never solved, and the switch
        k0, r0 = eng.get_ray([0])
        assert k0[0] == K_NONE and not r0.any()
        assert eng.certify_rays([0])["verdict"][0] == 15
        eng.reset_slot(1)
        assert eng.get_ray([1])[0][0] == K_NONE
        kind = np.zeros(1, np.int32)
        slot = np.array([2], np.int32)
        assert eng.lib.bslv_lpq_get_ray(eng.h, 1, slot.ctypes.data, kind.ctypes.data, None) == E_ARG          # (a pool of 2 slots)
        assert eng.lib.bslv_lpq_get_ray(eng.h, 0, None, None, None) == 0
        assert eng.set_rays(0) == 0 and eng.get_rays() == 0
        slot[0] = 1
        assert eng.lib.bslv_lpq_get_ray(eng.h, 1, slot.ctypes.data, kind.ctypes.data, None) == E_STATE
        st, _, _ = _solve(eng, [0], [1], EMPTY, EMPTY, form == "revised")
        assert st[0] == INFEASIBLE
    finally:
        eng.close()


# ---- 2. the boxed sets, every arm ------------------------------------------------------------------------------------------------
def _arms(form):
    for method in ((DUAL, PRIMAL) if form == "tableau" else (DUAL,)):
        for pricing in (DANTZIG, DEVEX):
            for ext in (0, 1):
                yield method, pricing, ext


@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("M,N", rc.SHAPES)
def test_boxed_sets(oracle, M, N, form):
    ref = rc.assert_boxed_references(M, N)
    s = rc.boxed_set(M, N)
    A, cost, vlo, vup, perm = s["A"], s["cost"], s["vlo"], s["vup"], s["perm"]
    retry = form == "revised"
    bad = list(BAD_LPS)
    eng = _ray_engine(A, s["lo"], s["up"], cost, 0, M, 1 + NLP, form)
    try:
        assert eng.rows_folded() == 0
        bytes0 = eng.slot_bytes()
        dst = np.arange(1, 1 + NLP, dtype=np.int32)
        for method, pricing, ext in _arms(form):
            tag = (form, M, N, "method", method, "pricing", pricing, "ext", ext)
            assert eng.set_method(method) == 0 and eng.set_pricing(pricing) == 0
            eng.set_extended(ext)
            eng.reset_slot(0)
            st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
            assert st[0] == OPTIMAL, (tag, st)
            st, _, _ = _solve(eng, np.zeros(NLP, np.int32), dst, vlo, vup, retry)
            assert np.array_equal(st, ref), (tag, st, ref)
            out = eng.certify_rays(dst, vlo, vup)
            assert eng.last_ray_certify_stats()["lps"] == NLP and eng.last_ray_certify_stats()["not_certified"] == NLP - len(bad)
            kinds, rays, host = _compare(eng, A, dst, lambda b: s["lps"][b], lambda b: cost, out, tag)
            for b in range(NLP):
                if b in bad:          # no exceptions: every column is boxed, no proof can lean on an artificial bound
                    assert kinds[b] == FARKAS and out["verdict"][b] == 0, (tag, b, kinds[b], out["verdict"][b], out["res"][b], out["at"][b])
                    assert np.abs(rays[b]).max() == 1.0
                else:
                    assert kinds[b] == K_NONE and out["verdict"][b] & 8, (tag, b, kinds[b], out["verdict"][b])
            # B = 1 and B = 17 (one slot named twice): the same bits as in the call of 16
            one = eng.certify_rays(dst[3:4], vlo[3:4], vup[3:4])
            assert np.array_equal(one["res"][0].view(np.uint64), out["res"][3].view(np.uint64)) and one["verdict"][0] == out["verdict"][3]
            sl17 = np.concatenate([dst, dst[5:6]])
            more = eng.certify_rays(sl17, np.vstack([vlo, vlo[5:6]]), np.vstack([vup, vup[5:6]]))
            assert np.array_equal(more["res"].view(np.uint64)[:NLP], out["res"].view(np.uint64)) and np.array_equal(more["verdict"][:NLP], out["verdict"])
            assert np.array_equal(more["res"][NLP].view(np.uint64), out["res"][5].view(np.uint64)) and more["verdict"][NLP] == out["verdict"][5]
            k17, r17 = eng.get_ray(sl17)
            assert np.array_equal(k17[:NLP], kinds) and np.array_equal(r17[NLP], rays[5])
            # the second generation, in place: LP perm[b] from the slot of LP b; a slot that was INFEASIBLE and is solved OPTIMAL has kind NONE again
            st2, _, _ = _solve(eng, dst, dst, vlo[perm], vup[perm], retry)
            assert np.array_equal(st2, ref[perm]), (tag, st2, ref[perm])
            k2, _ = eng.get_ray(dst)
            assert np.array_equal(k2 == FARKAS, ref[perm] == INFEASIBLE) and np.array_equal(k2 == K_NONE, ref[perm] == OPTIMAL), (tag, k2)
            assert all(k2[b] == K_NONE for b in bad if ref[perm[b]] == OPTIMAL) and any(ref[perm[b]] == OPTIMAL for b in bad)
            out2 = eng.certify_rays(dst, vlo[perm], vup[perm])
            _compare(eng, A, dst, lambda b: s["lps"][perm[b]], lambda b: cost, out2, tag + ("gen2",))
            assert all(out2["verdict"][b] == 0 for b in range(NLP) if ref[perm[b]] == INFEASIBLE), (tag, out2["verdict"])
        assert eng.slot_bytes() == bytes0
    finally:
        eng.close()


# ---- 3. the general sets: a column that starts on an artificial bound -------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", rc.SHAPES)
def test_general_sets_bad_lp(oracle, M, N, arr, form):
    s = lc.general_set(M, N, arr)
    rows, _ = lc.assert_references_agree(M, N, arr)
    assert rows[BAD]["st"] == INFEASIBLE
    A, cost, vlo, vup = s["A"], s["cost"], s["vlo"], s["vup"]
    retry = form == "revised"
    eng = _ray_engine(A, s["lo"], s["up"], cost, s["var_first"], s["var_cnt"], 2, form)
    try:
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
        assert st[0] == OPTIMAL
        one = slice(BAD, BAD + 1)
        st, _, _ = _solve(eng, [0], [1], vlo[one], vup[one], retry)
        assert st[0] == INFEASIBLE, st
        out = eng.certify_rays([1], vlo[one], vup[one])
        kinds, rays, host = _compare(eng, A, [1], lambda b: s["lps"][BAD], lambda b: cost, out, (form, M, N, arr))
        assert kinds[0] == FARKAS
        v, at = int(out["verdict"][0]), out["at"][0]
        print("lp_ray_cases general set %s M %d N %d arr %s LP %d: verdict %d res %s at %s" % (form, M, N, arr, BAD, v, out["res"][0].tolist(), at.tolist()))
        # column N - 1 starts on an artificial bound: a proof through it comes back open there, and nothing else may be wrong
        assert v == 0 or (v == 2 and at[1] == M + N - 1), (form, M, N, arr, v, out["res"][0], at)
    finally:
        eng.close()


# ---- 4. unbounded objectives: a direction -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("M,N", [(15, 16), (32, 65), (24, 1121)])
def test_unbounded_objectives_store_a_direction(oracle, M, N, form):
    s = lc.unbounded_objective_set(M, N)
    ref, _ = lc.unbounded_objective_references(M, N)
    A, first, C = s["A"], s["cost_first"], s["costs"]
    eng = _ray_engine(A, s["lo"], s["up"], s["cost"], 0, 0, 1 + NLP, form)
    try:
        _feasible_start(eng, 0, EMPTY, EMPTY)
        dst = np.arange(1, 1 + NLP, dtype=np.int32)
        st, _, _ = _solve_obj(eng, np.zeros(NLP, np.int32), dst, first, C, form == "revised")
        assert np.array_equal(st, [r["st"] for r in ref]), (st, [r["st"] for r in ref])
        assert eng.last_ray_stats()["direction"] >= len(lc.UNB_LPS)
        out = eng.certify_rays(dst, cost_first=first, costs=C)

        def cost_of(b):
            c = np.zeros(M + N)
            c[first:first + C.shape[1]] = C[b]
            return c
        kinds, rays, host = _compare(eng, A, dst, lambda b: (s["lo"], s["up"]), cost_of, out, (form, M, N, "unbounded objectives"))
        for t in range(NLP):
            if t in lc.UNB_LPS:
                e = np.zeros(M + N)
                e[M] = -lc.UNB_LPS[t]
                assert st[t] == UNBOUNDED and kinds[t] == DIRECTION and np.array_equal(rays[t], e), (t, kinds[t], rays[t][M])
                assert list(out["res"][t]) == [0.0, 0.0, 1.0, 1.0] and out["verdict"][t] == 0, (t, out["res"][t], out["verdict"][t])
            else:
                assert kinds[t] == K_NONE and out["verdict"][t] & 8
    finally:
        eng.close()


# ---- 5. UNBOUNDED on an artificial bound stores nothing; the primal method finds the direction -------------------------------------
@pytest.mark.parametrize("M,N", [(16, 17), (33, 257)])
def test_unbounded_model_dual_stores_nothing_primal_a_direction(M, N):
    A, lo, up, cost = lc.unbounded_model(M, N)
    eng = _ray_engine(A, lo, up, cost, 0, 0, 2, "tableau")
    try:
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [1], EMPTY, EMPTY)
        assert st[0] == UNBOUNDED, st
        assert eng.last_ray_stats()["none"] >= 1 and eng.last_ray_stats()["direction"] == 0
        kind, ray = eng.get_ray([1])
        out = eng.certify_rays([1])
        assert kind[0] == K_NONE and not ray.any() and out["verdict"][0] & 8, (kind, out)
        assert eng.set_method(PRIMAL) == 0
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [1], EMPTY, EMPTY)
        assert st[0] == UNBOUNDED, st
        assert eng.last_ray_stats()["direction"] == 1
        out = eng.certify_rays([1])
        kinds, rays, host = _compare(eng, A, [1], lambda b: (lo, up), lambda b: cost, out, ("unbounded model", M, N))
        print("lp_ray_cases unbounded model M %d N %d under PRIMAL: res %s" % (M, N, out["res"][0].tolist()))
        assert kinds[0] == DIRECTION and out["verdict"][0] == 0, (kinds, out)
    finally:
        eng.close()


# ---- 6. folded rows ----------------------------------------------------------------------------------------------------------------
def _folded_case():
    """boxed_set(15, 16) with two rows of a single non-zero added behind the per-LP range (a > 0 on column j1, a < 0 on column j2), each
    taking 1.5 off the upper bound of its column.  LP 0: the model's bounds.  LP 1: the rows around A x* for the vertex x* of the
    columns' own box that maximises row i, and row i >= a_i . x*: feasible without the two rows (x* itself), infeasible with them."""
    s = rc.boxed_set(15, 16)
    A, lo, up, tr = s["A"], s["lo"], s["up"], s["tr"]
    M, N = A.shape
    clo, cup = lo[M:], up[M:]
    i = next(i for i in range(M) if tr[i] in "lds" and (A[i] > 0).sum() >= 2)
    j1, j2 = [j for j in range(N) if A[i, j] > 0][:2]
    extra = np.zeros((2, N))
    extra[0, j1], extra[1, j2] = 2.0, -1.5
    A2 = np.vstack([A, extra])
    lo2 = np.concatenate([lo[:M], [-np.inf, -1.5 * (cup[j2] - 1.5)], clo])
    up2 = np.concatenate([up[:M], [2.0 * (cup[j1] - 1.5), np.inf], cup])
    xs = np.where(A[i] > 0, cup, clo)
    rng = np.random.default_rng(77)
    vlo, vup = np.tile(lo[:M], (2, 1)), np.tile(up[:M], (2, 1))
    vlo[1], vup[1] = lc._typed(tr, A @ xs, rng, 2)
    vlo[1, i] = float(A[i] @ xs)
    lps = []
    for t in range(2):
        l, u = lo2.copy(), up2.copy()
        l[:M], u[:M] = vlo[t], vup[t]
        lps.append((l, u))
    return A2, lo2, up2, s["cost"], M, vlo, vup, lps, i


@pytest.mark.parametrize("presolve", [True, False])
@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_folded_rows_ray_in_the_indices_of_the_model_as_given(form, presolve):
    A, lo, up, cost, Mr, vlo, vup, lps, i = _folded_case()
    M, N = A.shape
    assert lc.highs(A, lps[0][0], lps[0][1], cost)[0] == OPTIMAL and lc.highs(A, lps[1][0], lps[1][1], cost)[0] == INFEASIBLE
    free = (np.concatenate([lps[1][0][:Mr], [-np.inf, -np.inf], lps[1][0][M:]]), np.concatenate([lps[1][1][:Mr], [np.inf, np.inf], lps[1][1][M:]]))
    assert lc.highs(A, free[0], free[1], cost)[0] == OPTIMAL          # (infeasible only through the two rows)
    with _env(BSLV_NO_PRESOLVE=None if presolve else "1"):
        eng = _ray_engine(A, lo, up, cost, 0, Mr, 3, form)
    try:
        assert eng.rows_folded() == (2 if presolve else 0)
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], form == "revised")
        assert st[0] == OPTIMAL
        dst = np.array([1, 2], np.int32)
        st, _, _ = _solve(eng, [0, 0], dst, vlo, vup, form == "revised")
        assert list(st) == [OPTIMAL, INFEASIBLE], st
        out = eng.certify_rays(dst, vlo, vup)
        kinds, rays, host = _compare(eng, A, dst, lambda b: lps[b], lambda b: cost, out, (form, "folded", presolve))
        print("lp_ray_cases folded rows %s presolve %s: ray on the two rows %s, res %s" % (form, presolve, rays[1][Mr:M].tolist(), out["res"][1].tolist()))
        assert list(kinds) == [K_NONE, FARKAS] and out["verdict"][1] == 0, (kinds, out)
        assert rays.shape[1] == M + N and np.any(rays[1][Mr:M] != 0.0), rays[1][Mr:M]          # the proof needs a bound only those rows give
    finally:
        eng.close()


# ---- 7. read-only, and off against on ----------------------------------------------------------------------------------------------
def _record(M, N, form, rays, certify):
    s = rc.boxed_set(M, N)
    vlo, vup, perm = s["vlo"], s["vup"], s["perm"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, M, 1 + 2 * NLP, form)
    try:
        if rays:
            assert eng.set_rays(1) == 0
        n = M + N
        eng.reset_slot(0)
        _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
        g1, g2 = np.arange(1, 1 + NLP, dtype=np.int32), np.arange(1 + NLP, 1 + 2 * NLP, dtype=np.int32)
        st1, it1, _ = _solve(eng, np.zeros(NLP, np.int32), g1, vlo, vup, retry)
        if certify:
            eng.certify_rays(g1, vlo, vup)
            eng.get_ray(g1)
        st2, it2, _ = _solve(eng, g1, g2, vlo[perm], vup[perm], retry)
        both = np.concatenate([g1, g2])
        return [np.concatenate([st1, st2]), np.concatenate([it1, it2]), eng.primal(both, 0, n).view(np.uint64), eng.dual(both, 0, n).view(np.uint64)]
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_read_only_and_off_against_on(form):
    M, N = 32, 65
    with_call, without, off = _record(M, N, form, True, True), _record(M, N, form, True, False), _record(M, N, form, False, False)
    for a, b, c in zip(with_call, without, off):
        assert np.array_equal(a, b) and np.array_equal(b, c)


# ---- 8. a damaged inverse ----------------------------------------------------------------------------------------------------------
def test_damaged_inverse_of_the_parent():
    M, N = 32, 65
    s = rc.boxed_set(M, N)
    vlo, vup = s["vlo"], s["vup"]
    eng = _ray_engine(s["A"], s["lo"], s["up"], s["cost"], 0, M, 2, "revised")
    try:
        eng.reset_slot(0)
        st, _, _ = _solve(eng, [0], [0], vlo[:1], vup[:1], True)
        assert st[0] == OPTIMAL
        eng.debug_perturb_inverse(0, 1e-6)
        t = BAD_LPS[0]
        one = slice(t, t + 1)
        st, _ = eng.solve_batch([0], [1], vlo[one], vup[one])
        out = eng.certify_rays([1], vlo[one], vup[one])
        kinds, rays, host = _compare(eng, s["A"], [1], lambda b: s["lps"][t], lambda b: s["cost"], out, ("damage",))
        print("lp_ray_cases damaged parent (revised, rel 1e-6): status %d kind %d verdict %d (yardstick %d) res %s at %s" % (
            st[0], kinds[0], out["verdict"][0], host[0]["verdict"], out["res"][0].tolist(), out["at"][0].tolist()))
        assert int(out["verdict"][0]) == host[0]["verdict"]
        assert (kinds[0] == K_NONE) == (st[0] != INFEASIBLE)
    finally:
        eng.close()


# ---- 9. the command-line driver -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex,frag,word", [("ex02", "VLP is infeasible", None), ("ex04", "totally unbounded", "not certified")])
def test_cli_says_what_the_ray_proves(tmp_path, ex, frag, word):
    cmd = [CLI, os.path.join(EXDIR, ex + ".vlp"), "-m", "1", "-o", os.path.join(tmp_path, ex)]
    env = {k: v for k, v in os.environ.items() if k != "BSLV_LP_RAYS"}
    off = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    on = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, BSLV_LP_RAYS="1"))
    for r in (off, on):
        assert r.returncode == 1 and frag in r.stdout, r.stdout + r.stderr
    assert "BSLV_LP_RAYS" not in off.stderr
    lines = [l for l in on.stderr.splitlines() if l.startswith("BSLV_LP_RAYS:")]
    assert len(lines) == 1, on.stderr
    assert [l for l in on.stderr.splitlines() if not l.startswith("BSLV_LP_RAYS:")] == off.stderr.splitlines()
    line = lines[0]
    print("lp_ray_cases cli %s: %s" % (ex, line))
    assert "ray kind" in line and line.count("e+") + line.count("e-") + line.count("nan") >= 4 and ("certified" in line), line
    if word:
        assert word in line, line
