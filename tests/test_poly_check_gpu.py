"""GPU: bslv_poly_check, the device-side consistency check of the resident polyhedron (poly__polyck, bslv_poly.c:940-990, and its
converse), against a numpy restatement of the same audit applied to the same dump.

audit() below is that restatement: the incidence matrix from dump()["I"], edge_test (bslv_poly.c:467-512) over all pairs, residuals
from Y and the v2h rule.  Every expected count comes from it, never from the code under test."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import poly_harness as ph
from bensolve_amd import synth
from bensolve_amd._lib import BslvError, load_library
from bensolve_amd.poly import PolyEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "poly_ref.npz"))
DEFECTS = (3, 4, 5, 7, 8, 10, 11)
POLY_EPS = 1e-9


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def v2h_map(v2h, c, v, is_dir):
    """dualV2primalH: cone_polar (bslv_poly.c:30-39), lowerV2upperH (bslv_algs.c:287-305), upperV2lowerH (bslv_algs.c:307-313)"""
    d = len(v)
    hp = np.zeros(d + 1)
    if v2h == 0:
        hp[:d] = v
        hp[d] = 0.0 if is_dir else -1.0
    elif v2h == 1:
        if is_dir:
            hp[d] = -1.0
        else:
            hp[:d - 1] = v[:d - 1]
            hp[d - 1] = 1.0 - c[:d - 1] @ v[:d - 1]
            hp[d] = v[d - 1]
    else:
        hp[d - 1] = 0.0 if is_dir else -1.0
        hp[:d - 1] = v[:d - 1] - v[d - 1] * c[:d - 1]
        hp[d] = -v[d - 1]
    return hp


def audit(dump, v2h=0, c=None, tol=1e-6, rows=None):
    """-> (the twelve counts of bslv_poly_check, the sorted offenders (kind, a, b), (largest listed residual, most negative slack))"""
    d = dump["d"]
    pu, pi, X = dump["pu"].astype(bool), dump["pi"].astype(bool), dump["X"]
    du, di, Y = dump["du"].astype(bool), dump["di"].astype(bool), dump["Y"]
    nv, nf = len(pu), len(du)
    c = np.zeros(d) if c is None else np.asarray(c, float)
    live = np.nonzero(pu)[0]
    L = len(live)
    rowof = -np.ones(nv, np.int64)
    rowof[live] = np.arange(L)
    first, count = (0, L) if rows is None else rows
    if count < 0:
        count = L - first
    H = np.array([v2h_map(v2h, c, Y[f], di[f]) for f in range(nf)])
    nogeo = np.zeros(nf, bool)
    nogeo[0] = di[0]                                   # the facet at infinity has no hyperplane of its own
    I = dump["I"].reshape(-1, 2)
    M = np.zeros((L, nf), bool)
    M[rowof[I[:, 0]], I[:, 1]] = True
    S = X[live] @ H[:, :d].T - np.where(pi[live][:, None], 0.0, H[:, d][None, :])          # slack of every live element, every dual slot
    off, worst_res = [], 0.0
    for a, f in I:
        res = 0.0 if nogeo[f] else abs(S[rowof[a], f])
        if du[f] and not nogeo[f]:
            worst_res = max(worst_res, res)
        if not du[f] or not res <= tol:
            off.append((3, int(a), int(f)))
    geo = np.nonzero(du & ~nogeo)[0]
    for r, f in np.argwhere((np.abs(S[:, geo]) <= POLY_EPS) & ~M[:, geo]):
        off.append((4, int(live[r]), int(geo[f])))
    worst_neg = 0.0
    for r, f in np.argwhere(S[:, geo] < -tol):
        off.append((5, int(live[r]), int(geo[f])))
        worst_neg = min(worst_neg, S[r, geo[f]])
    E = dump["E"].reshape(-1, 2)
    edges = set()
    for a, b in E:
        if a < 0 or b < 0 or a >= nv or b >= nv or a == b or not pu[a] or not pu[b]:
            off.append((7, int(a), int(b)))
        elif (min(a, b), max(a, b)) in edges:
            off.append((8, int(min(a, b)), int(max(a, b))))
        else:
            edges.add((int(min(a, b)), int(max(a, b))))
    Mi = M.astype(np.int32)
    common = Mi @ Mi.T
    cand = np.triu(common >= d - 1, 1) if d > 1 else np.triu(np.ones((L, L), bool), 1)
    passing = set()
    for i, j in np.argwhere(cand):
        if not first <= i < first + count:
            continue
        mutual = M[i] & M[j]
        sup = Mi[:, mutual].sum(1) == mutual.sum()          # elements on every mutual facet (bslv_poly.c:487-505)
        sup[i] = sup[j] = False
        if d == 1 or not sup.any():
            passing.add((int(live[i]), int(live[j])))
    listed = {e for e in edges if first <= rowof[e[0]] < first + count}
    off += [(10, a, b) for a, b in passing - listed] + [(11, a, b) for a, b in listed - passing]
    n = lambda k: sum(1 for o in off if o[0] == k)
    out = [L, int(du.sum()), len(I), n(3), n(4), n(5), len(E), n(7), n(8), len(passing), n(10), n(11)]
    return out, sorted(off), (worst_res, worst_neg)


# ---- building the cases --------------------------------------------------------------------------------------------------------
def build_golden(name, batched):
    """a case of tests/golden/poly_ref.npz: one bslv_poly_add per cut, or (batched) the cuts after the initial cone as ONE
    bslv_poly_add_cuts (rounds of independent cuts, hot mode)"""
    q, v2h, apex, init_after = [int(x) for x in GOLD[name + "/in_meta"]]
    vals, ideals = GOLD[name + "/in_vals"], [int(x) for x in GOLD[name + "/in_ideals"]]
    G = PolyEngine(q, v2h)
    if apex:
        G.dual0_apex()
    if not batched:
        ph.run_sequence(G, vals, ideals, None if init_after < 0 else init_after)
    else:
        k0 = init_after if init_after >= 0 else min(len(vals), 2 * q + 2)
        for k in range(k0):
            G.add(vals[k], ideals[k])
        assert G.init() == 0
        if k0 < len(vals):
            G.add_cuts(vals[k0:], np.asarray(ideals[k0:]))
    return G, v2h


def join_duals(n):
    """the join of two regular n-gons in R^5 through cone_polar: a pair of its vertices lies on 2 (n - 2) >= d - 1 common facets
    and still is no edge when both belong to the same polygon and are not neighbours there -- the branch of edge_test that removes
    a candidate pair, which no case of poly_ref.npz takes"""
    k = np.arange(n)
    u = np.stack([np.cos(2 * np.pi * (k + 0.5) / n), np.sin(2 * np.pi * (k + 0.5) / n)], 1)
    z = np.zeros((n, 2))
    return np.vstack([np.hstack([-2 * u, z, np.ones((n, 1))]), np.hstack([z, -2 * u, -np.ones((n, 1))])])


def build_join(n):
    G = PolyEngine(5)
    ph.run_sequence(G, join_duals(n))
    return G


def sha(dump):
    hh = hashlib.sha256()
    for k in ("pu", "pi", "ps", "X", "du", "di", "Y", "E", "I"):
        hh.update(np.ascontiguousarray(dump[k]).tobytes())
    return hh.hexdigest()


def assert_matches_restatement(G, v2h=0, c=None, rows=None, max_offenders=4096):
    got = G.check(rows=rows, max_offenders=max_offenders)
    exp_out, exp_off, exp_worst = audit(G.dump(), v2h, c, rows=rows)
    print("check", got["out"], "restatement", exp_out, "worst", got["worst"], exp_worst)
    assert got["out"] == exp_out
    assert got["n_offenders"] == len(exp_off) and got["offenders"] == exp_off
    assert abs(got["worst"][0] - exp_worst[0]) <= 1e-12 * max(1.0, exp_worst[0]) + 1e-13
    assert abs(got["worst"][1] - exp_worst[1]) <= 1e-12 * max(1.0, -exp_worst[1]) + 1e-13
    return got


def assert_clean(got):
    assert [got["out"][k] for k in DEFECTS] == [0] * len(DEFECTS), got
    assert got["out"][9] == got["out"][6] and got["clean"] and got["n_offenders"] == 0 and got["offenders"] == []


# ---- 1. clean states ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("name", ["cube_q3", "cone_ex05", "cross_q5", "tangent_q2_N25", "tangent_q5_N120"])
def test_clean_states_report_all_zeros(name, batched):
    G, v2h = build_golden(name, batched)
    got = assert_matches_restatement(G, v2h)
    assert_clean(got)
    assert got["worst"][0] < 1e-9 and got["worst"][1] == 0.0
    G.close()


def test_clean_at_survey_size():
    """SURVEY 8c's size (27 418 elements at q = 5, N = 1000; a full check takes about 15 ms there, profiles/poly_check_cost.txt): more
    than one slab of 2^20 pair blocks.  The numpy restatement is quadratic in memory, so the expected counts are the reference's own,
    recorded with the fixture: elements, facets, incidences and edges of tests/golden/poly_ref_large.*; every defect count is zero."""
    import json
    gold = np.load(os.path.join(ROOT, "tests", "golden", "poly_ref_large.npz"))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "poly_ref_large.json")))
    name = "tangent_q5_N1000"
    q, v2h, apex, init_after = [int(x) for x in gold[name + "/in_meta"]]
    vals = gold[name + "/in_vals"]
    G = PolyEngine(q, v2h)
    for k in range(init_after):
        G.add(vals[k])
    assert G.init() == 0
    G.add_cuts(vals[init_after:])
    got = G.check()
    print("check", got["out"], "worst", got["worst"])
    assert_clean(got)
    assert got["out"][0] == len(gold[name + "/X"]) and got["out"][1] == len(gold[name + "/Y"])
    assert got["out"][2] == meta[name]["I"][1] and got["out"][6] == meta[name]["E"][1] == got["out"][9]
    assert got["worst"][0] < 1e-9 and got["worst"][1] == 0.0
    G.close()


def solve_primal_keep(ex):
    """bslv_vlp_solve_primal on a committed example; returns (the finished engine, its polyhedron as a PolyEngine view, c of the
    engine's lowerV2upperH)"""
    from bensolve_amd.vlp import VlpInfo
    from bensolve_amd.poly import _bind
    lib = load_library()
    _bind(lib)
    prob = synth.read_vlp(os.path.join(ROOT, "tests", "golden", "ex", ex + ".vlp"))
    vp = ctypes.c_void_p
    f8 = lambda a: np.ascontiguousarray(a, np.float64)
    A, P, rt, ct = f8(prob["A"]), f8(prob["P"]), np.ascontiguousarray(prob["rtype"], np.uint8), np.ascontiguousarray(prob["ctype"], np.uint8)
    b = [f8(prob[k]) for k in ("rlb", "rub", "clb", "cub")]
    gen = None if prob["gen"] is None else f8(prob["gen"])
    cin = f8(prob["c"]) if np.any(prob["c"]) else None
    h, st, info = vp(), ctypes.c_int(), VlpInfo()
    lib.bslv_vlp_solve_primal.argtypes = [ctypes.c_int] * 3 + [vp] * 8 + [ctypes.c_int] * 2 + [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int] + [ctypes.c_double] * 4 + [ctypes.c_int, vp, vp, vp]
    rc = lib.bslv_vlp_solve_primal(prob["m"], prob["n"], prob["q"], A.ctypes.data, P.ctypes.data, rt.ctypes.data, b[0].ctypes.data, b[1].ctypes.data, ct.ctypes.data,
                                   b[2].ctypes.data, b[3].ctypes.data, prob["optdir"], prob["cone_kind"], None if gen is None else gen.ctypes.data,
                                   0 if gen is None else gen.shape[1], None if cin is None else cin.ctypes.data, 0, 0, 1e-8, 1e-8, 1e-7, 1e-7, 64,
                                   ctypes.byref(h), ctypes.byref(st), ctypes.byref(info))
    assert rc == 0 and st.value == 4, (rc, st.value, lib.bslv_last_error())
    q = prob["q"]
    c = np.ctypeslib.as_array(info.c, shape=(q,)).copy() * info.c_dir
    lib.bslv_vlp_info_free.argtypes = [vp]
    lib.bslv_vlp_info_free.restype = None
    lib.bslv_vlp_info_free(ctypes.byref(info))
    lib.bslv_benson_poly.restype = vp
    lib.bslv_benson_poly.argtypes = [vp]
    pe = PolyEngine.__new__(PolyEngine)
    pe.lib, pe.h, pe.d = lib, vp(lib.bslv_benson_poly(h)), q
    return h, pe, c


@pytest.mark.parametrize("ex", ["ex01", "ex05"])
def test_upper_image_of_a_finished_run_is_clean(ex):
    """v2h = 1 (lowerV2upperH): ex01 has an unbounded upper image, ex05 an ordering cone given by generators"""
    h, pe, c = solve_primal_keep(ex)
    try:
        got = assert_matches_restatement(pe, 1, c)
        assert_clean(got)
    finally:
        pe.h = None
        lib = load_library()
        lib.bslv_benson_destroy.argtypes = [ctypes.c_void_p]
        lib.bslv_benson_destroy.restype = None
        lib.bslv_benson_destroy(h)


# ---- 2. the elimination branch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,elements,candidates,edges,longest", [(4, 8, 28, 24, None), (40, 80, 3160, 1680, None), (70, 140, 9730, 5040, 72)])
def test_join_of_two_polygons_takes_the_elimination_branch(n, elements, candidates, edges, longest):
    """candidate pairs that are NOT edges: a kernel that skips the superset sweep would report candidates - edges of them"""
    G = build_join(n)
    d = G.dump()
    live = np.nonzero(d["pu"])[0]
    M = np.zeros((len(d["pu"]), len(d["du"])), np.int32)
    M[d["I"][:, 0], d["I"][:, 1]] = 1
    common = (M[live] @ M[live].T)
    assert len(live) == elements and int(np.triu(common >= 4, 1).sum()) == candidates
    if longest:
        assert M.sum(1).max() == longest          # (past the 64 entries from which the engine's list code is wave-cooperative)
    got = assert_matches_restatement(G)
    assert_clean(got)
    assert got["out"][9] == edges
    G.close()


# ---- 3. each defect is seen, and only it ---------------------------------------------------------------------------------------
def _base(which):
    return build_golden("cube_q3", False)[0] if which == "cube_q3" else build_join(4)


def _non_edge(d):
    live = np.nonzero(d["pu"])[0]
    have = {tuple(sorted(e)) for e in d["E"]}
    return next((int(a), int(b)) for a in live for b in live if a < b and (a, b) not in have)


CORRUPTIONS = ["deleted_edge", "appended_non_edge", "appended_existing_edge", "dropped_incidence", "coordinate_plus", "coordinate_minus"]


@pytest.mark.parametrize("how", CORRUPTIONS)
@pytest.mark.parametrize("which", ["cube_q3", "join4"])
def test_each_defect_is_seen_and_only_it(which, how):
    G = _base(which)
    d0 = G.dump()
    assert_clean(G.check())
    live = np.nonzero(d0["pu"])[0]
    only = None                                # the defect counts that move, where nothing else can
    if how == "deleted_edge":
        G.debug_corrupt(0, 1)
        only = {10: 1}
    elif how == "appended_non_edge":
        G.debug_corrupt(1, *_non_edge(d0))
        only = {11: 1}
    elif how == "appended_existing_edge":
        G.debug_corrupt(1, int(d0["E"][2][1]), int(d0["E"][2][0]))          # (the same unordered pair, endpoints swapped)
        only = {8: 1}
    elif how == "dropped_incidence":
        G.debug_corrupt(2, int(live[1]))
    else:
        G.debug_corrupt(3, int(live[2]), 1, 1e-3 if how == "coordinate_plus" else -1e-3)
    got = assert_matches_restatement(G)          # all twelve counts and the sorted offenders are those of the damaged dump
    assert not got["clean"]
    if only is not None:
        assert {k: got["out"][k] for k in DEFECTS if got["out"][k]} == only
    elif how == "dropped_incidence":             # the element still lies on the facet it no longer lists; its edges through that facet now fail the test
        assert got["out"][4] == 1 and got["out"][3] == 0 and got["out"][5] == 0
    else:                                        # the element left the hyperplanes it lists by about 1e-3
        assert got["out"][3] >= 1 and got["out"][4] == 0 and got["worst"][0] > 1e-4
    G.close()


def test_the_check_is_read_only():
    """an engine that is checked after every cut ends bit-identical to one that never was"""
    q, v2h, apex, init_after = [int(x) for x in GOLD["tangent_q4_N100/in_meta"]]
    vals = GOLD["tangent_q4_N100/in_vals"]
    digests = []
    for checked in (False, True):
        G = PolyEngine(q, v2h)
        for k in range(init_after):
            G.add(vals[k])
        assert G.init() == 0
        for k in range(init_after, 40):
            G.add(vals[k])
            if checked:
                G.check()
        G.add_cuts(vals[40:70])
        if checked:
            G.check(rows=(3, 5))
        G.add_cuts(vals[70:])
        if checked:
            assert_clean(G.check())
        digests.append((sha(G.dump()), G.counts(), G.path_stats(), G.rounds2_stats()))
        G.close()
    assert digests[0] == digests[1]


# ---- 4. row ranges -------------------------------------------------------------------------------------------------------------
def test_row_ranges_add_up():
    G, v2h = build_golden("tangent_q4_N100", False)
    full = G.check()
    L = full["out"][0]
    assert L > 300
    parts = [G.check(rows=r) for r in ((0, 100), (100, 200), (300, L - 300))]
    for k in (9, 10, 11):
        assert sum(p["out"][k] for p in parts) == full["out"][k]
    for p in parts:
        assert p["out"][:9] == full["out"][:9]
    exp_out, _, _ = audit(G.dump(), v2h, rows=(100, 200))
    assert parts[1]["out"] == exp_out
    empty = G.check(rows=(17, 0))
    assert empty["out"][9:] == [0, 0, 0] and empty["out"][:9] == full["out"][:9]
    # a damaged polyhedron: the extra edge is counted under the row of its smaller endpoint, the missing one under its row
    a, b = _non_edge(G.dump())
    G.debug_corrupt(1, b, a)
    G.debug_corrupt(0, 0)
    full = G.check()
    assert full["out"][10] == 1 and full["out"][11] == 1
    parts = [G.check(rows=r) for r in ((0, 100), (100, 200), (300, L - 300))]
    for k in (9, 10, 11):
        assert sum(p["out"][k] for p in parts) == full["out"][k]
    G.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = load_library()
    out = (ctypes.c_long * 12)()
    lib.bslv_poly_check.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.bslv_poly_debug_corrupt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert lib.bslv_poly_check(None, 0.0, 0, -1, out, None, None, 0, None) == 2            # BSLV_E_ARG
    assert lib.bslv_poly_debug_corrupt(None, 0, 0, 0, 0.0) == 2
    G = PolyEngine(3)
    for v in np.vstack([np.eye(3), -np.eye(3)]):
        G.add(v)
    with pytest.raises(BslvError, match="error 5"):                                            # BSLV_E_STATE: before bslv_poly_init
        G.check()
    assert G.init() == 0
    L = G.check()["out"][0]
    assert L == 8
    for rows in ((-1, 1), (L + 1, 0), (0, L + 1), (L - 1, 2)):
        with pytest.raises(BslvError, match="error 2"):
            G.check(rows=rows)
    assert G.check(rows=(L, 0))["out"][9:] == [0, 0, 0]
    with pytest.raises(BslvError, match="error 2"):
        G.check(max_offenders=-1)
    ne, nv = G.counts()["nedges"], G.counts()["nprimal"]
    for args in ((0, ne), (0, -1), (1, nv, 0), (1, 0, -1), (2, nv), (2, -1), (3, nv, 0, 1.0), (3, 0, 3, 1.0), (3, 0, -1, 1.0), (4, 0), (-1, 0)):
        with pytest.raises(BslvError, match="error 2"):
            G.debug_corrupt(*args)
    assert_clean(G.check())                    # (the refused calls changed nothing)
    G.close()


# ---- 6. -t on the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ex", ["ex01", "ex05"])
def test_cli_test_option_audits_the_result(tmp_path, ex):
    cli = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
    vlp = os.path.join(ROOT, "tests", "golden", "ex", ex + ".vlp")
    runs = {}
    for tag, extra in (("plain", []), ("test", ["-t"])):
        base = os.path.join(tmp_path, tag)
        r = subprocess.run([cli, vlp, "-m", "1", "-o", base] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = (r.stdout, {f[len(tag):]: open(os.path.join(tmp_path, f), "rb").read() for f in sorted(os.listdir(tmp_path)) if f.startswith(tag) and f.endswith(".sol")})
    lines = [l for l in runs["test"][0].splitlines() if l.startswith("polyhedron check:")]
    assert len(lines) == 1 and lines[0].endswith("ok"), runs["test"][0]
    assert not [l for l in runs["plain"][0].splitlines() if l.startswith("polyhedron check:")]
    assert runs["plain"][1] and runs["plain"][1] == runs["test"][1]


def test_driver_audits_after_every_outer_iteration(tmp_path):
    """BSLV_POLY_CHECK=1: the Benson driver runs the check after every apply() and leaves a tally on stderr when an engine is
    destroyed (ex05: the homogeneous engine of phase 1 and the engine of phase 2); without the switch it prints nothing"""
    import re
    cli = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
    vlp = os.path.join(ROOT, "tests", "golden", "ex", "ex05.vlp")
    outs = {}
    for on in ("0", "1"):
        base = os.path.join(tmp_path, "on" + on)
        r = subprocess.run([cli, vlp, "-m", "0", "-o", base], env=dict(os.environ, BSLV_POLY_CHECK=on), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[on] = ([l for l in r.stderr.splitlines() if l.startswith("BSLV_POLY_CHECK:")], open(base + "_img_p.sol", "rb").read())
    assert outs["0"][0] == [] and outs["0"][1] == outs["1"][1]
    tallies = [re.match(r"BSLV_POLY_CHECK: (\d+) audits after (\d+) outer iterations.*?, (\d+) not clean", l) for l in outs["1"][0]]
    tallies = [m for m in tallies if m]
    print("\n".join(outs["1"][0]))
    assert len(tallies) >= 2 and sum(int(m.group(1)) for m in tallies) > 0
    for m in tallies:
        assert m.group(1) == m.group(2) and m.group(3) == "0", outs["1"][0]
