"""GPU: every dimension instance of the polyhedron kernels, d = 2 .. 16, against the CPU oracle (oracle/poly_dd.c).

k_emit2<D>, k_classify_batch_t<D, .>, k_r2_emit<D>, k_r2_classify3<D> and k_r2_prune_classify<D> are compiled for D = 2 .. 10 and
once more (D = 0, register arrays of MAXD = 16 doubles) for d = 11 .. 16.  Incidence lists of up to LCAP = 16 facets are intersected in
registers, longer ones take match_mask_long, the bitmap or (past LONGN = 64) the wave-cooperative path.  The cases (generators in
poly_harness.py) put ordinary elements on every side of those boundaries:
  truncated simplex, every d   simple vertices, every list exactly d long (= LCAP at d = 16)
  cube 7, 9, 10, 12            up to 4096 simple vertices
  truncated cube 7             672 vertices on 9 facets: degenerate, below LCAP
  cross-polytope 7, 8          vertices on 64 (= LONGN) and 128 facets
  tangent halfspaces 7, 9      3924 / 5936 simple vertices
  ideal generators 7, 11, 16   cones (dual0_apex), lists of up to 9 / 18 / 27
  degenerate simplex 11, 16    ordinary vertices on d + 1 .. d + 4 facets: at d = 16 lists of 17 .. 20, one step past LCAP
The oracle itself is pinned against the compiled reference at these dimensions by tests/golden/poly_ref_dims.npz
(tests/test_oracle_poly.py); the engine is compared with that fixture too at d = 10 and 16."""
import functools
import json
import os

import numpy as np
import pytest

import poly_harness as ph
from bensolve_amd._lib import load_library
from bensolve_amd.poly import PolyEngine, _bind
from test_poly_gpu import run_both, assert_slotwise_equal
from test_poly_modes_gpu import hooks, MODES, gpu_run
from test_r2_ride_gpu import ride_hooks
from test_poly_check_gpu import assert_matches_restatement, assert_clean

pytestmark = pytest.mark.gpu

DIMS = list(range(2, 17))
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the cases: name -> (q, vals, ideals, apex, init_after of the sequential run, k0 of a batched run or None) -------------------
def _cases():
    cases = {}
    for q in DIMS:
        vals, k0 = ph.truncated_simplex(q, 2 * (q + 1), 5)
        cases["truncated simplex q%d" % q] = (q, vals, None, False, k0, k0)
    for q in (7, 9, 10, 12):
        cases["cube q%d" % q] = (q, ph.cube(q), None, False, None, q + 1)
    cases["truncated cube q7"] = (7, ph.truncated_cube(7), None, False, None, 16)
    for q in (7, 8):
        S = ph.sign_vectors(q)
        cases["cross-polytope q%d" % q] = (q, S, None, False, None, None)
        # (the first sign vectors differ in their last coordinates only: a batched run needs a start of full rank)
        cases["cross-polytope q%d, shuffled" % q] = (q, S[np.random.default_rng(q).permutation(len(S))], None, False, None, 2 * q + 2)
    for q, N in ((7, 30), (9, 14)):
        cases["tangent q%d" % q] = (q, ph.tangent_halfspaces(q, N + q + 3, q), None, False, q + 3, q + 3)
    for q in (7, 11, 16):
        G = ph.ideal_cone(q, 3)
        cases["ideal cone q%d" % q] = (q, G, [1] * len(G), True, None, q + 2)
    for q in (11, 16):
        vals, k0 = ph.degenerate_simplex(q, 0)
        cases["degenerate simplex q%d" % q] = (q, vals, None, False, k0, k0)
    return cases


CASES = _cases()
NAMES = list(CASES)
BATCHED = [n for n in NAMES if CASES[n][5] is not None]


def _oracle(q, vals, ideals, apex, init_after, v2h=0, c=None):
    O = ph.FlatPoly("oracle", q, v2h, c)
    if apex:
        O.dual0_apex()
    rcs = ph.run_sequence(O, vals, ideals, init_after)
    O.dual_adjacency()
    d = O.dump()
    O.close()
    return [int(r) for r in rcs], d


@functools.lru_cache(maxsize=None)
def oracle_run(name, batched=False):
    """(return codes, dump) of the oracle; batched: initialised after k0 as the batched engine runs are.  Read-only for its users."""
    q, vals, ideals, apex, init_after, k0 = CASES[name]
    return _oracle(q, vals, ideals, apex, k0 if batched else init_after)


@functools.lru_cache(maxsize=None)
def oracle_canonical(name):
    return ph.canonical(oracle_run(name, True)[1])


def list_lengths(d):
    """incident facets of every live non-ideal element"""
    pts = d["pu"].astype(bool) & (d["pi"] == 0)
    return np.bincount(d["I"][:, 0], minlength=len(pts))[pts]


# ---- part 1's conditions on the degenerate polytopes, on the oracle ---------------------------------------------------------------
def test_degenerate_simplex_has_ordinary_vertices_past_the_register_lists():
    import time
    t0 = time.perf_counter()
    rcs, d = _oracle(*CASES["degenerate simplex q16"][:5])
    seconds = time.perf_counter() - t0
    n = list_lengths(d)
    print("d = 16: %d live vertices, %d on more than 16 facets, %d on exactly 17, longest list %d, oracle %.2f s" % (
        len(n), (n > 16).sum(), (n == 17).sum(), n.max(), seconds))
    assert (n > 16).sum() >= 20 and (n == 17).sum() >= 1
    assert not any(rcs)                                   # no cut of the sequence is redundant
    assert seconds < 2.0
    rcs, d = oracle_run("degenerate simplex q11")
    n = list_lengths(d)
    assert (n > 11).sum() >= 20 and (n == 12).sum() >= 1 and not any(rcs)
    # the other boundaries the cases are there for
    assert set(list_lengths(oracle_run("cross-polytope q7")[1])) == {64}            # = LONGN
    assert set(list_lengths(oracle_run("cross-polytope q8")[1])) == {128}
    assert set(list_lengths(oracle_run("truncated cube q7")[1])) == {9}
    assert set(list_lengths(oracle_run("truncated simplex q16")[1])) == {16}        # = LCAP
    assert int(oracle_run("cube q12")[1]["pu"].sum()) == 4096


# ---- (a) the sequential path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sequential_path_matches_oracle_slotwise(name):
    """one bslv_poly_add per cut, and the cuts after the start as one bslv_poly_add_cuts in batch mode 0 (index order, hot chunks):
    flags, edges, incidence and dual adjacency exact, coordinates 1e-12 (test_poly_gpu's rule)"""
    q, vals, ideals, apex, init_after, k0 = CASES[name]
    do, dg = run_both(q, vals, ideals, init_after, apex=apex)
    assert_slotwise_equal(do, dg)
    if k0 is not None:
        do, dg = run_both(q, vals, ideals, k0, apex=apex, batched=True, mode=0)
        assert_slotwise_equal(do, dg)


# ---- (b) rounds of independent cuts -----------------------------------------------------------------------------------------------
ALWAYS = {"BSLV_R2_MIN_CUTS": "-1"}
ARMS = {
    "default": ({}, True),
    "rounds always": (dict(ALWAYS), True),
    "rounds always, every prune through the multi-kernel path": (dict(ALWAYS, BSLV_K2_LDS="64"), True),
    "rounds always, local minima of one random order": (dict(ALWAYS, BSLV_R2_MIS="0"), True),
    "new vertices classified in a launch of their own": ({}, False),
}
R2_MIN_BATCH = 16            # a chunk goes to the device-selected rounds from 16 cuts that remove something (run_sequence)


def rounds_run(name, env, ride):
    q, vals, ideals, apex, init_after, k0 = CASES[name]
    vals = np.asarray(vals, float)
    idl = np.zeros(len(vals), np.int32) if ideals is None else np.asarray(ideals, np.int32)
    with (hooks(env) if ride else ride_hooks(env, False)):
        G = PolyEngine(q, 0, None)
        if apex:
            G.dual0_apex()
        rcs = [G.add(vals[i], int(idl[i])) for i in range(k0)]
        assert G.init() == 0
        rcs += list(G.add_cuts(vals[k0:], idl[k0:]))
        G.dual_adjacency()
        d, st, health = G.dump(), G.rounds2_stats(), G.rounds2_health()
        G.close()
    return [int(r) for r in rcs], d, st, health


@pytest.mark.parametrize("name", BATCHED)
def test_rounds_build_the_oracles_polyhedron(name):
    """bslv_poly_add_cuts in batch mode 1, five arms: vertices, facets, incidence, adjacency and dual adjacency are the oracle's as
    sets (poly_harness.assert_same at its defaults).  Whether a batch reaches the device-selected rounds is decided by the oracle's
    return codes alone: at least 16 cuts of it remove something."""
    q, vals, ideals, apex, init_after, k0 = CASES[name]
    rco, _ = oracle_run(name, True)
    reaches = len(rco) - k0 - sum(rco[k0:]) >= R2_MIN_BATCH
    if name.startswith("truncated simplex"):
        assert reaches == (q >= 7)                    # every dimension from 7 on runs the rounds' kernels
    exp = oracle_canonical(name)
    for arm, (env, ride) in ARMS.items():
        rcs, d, st, health = rounds_run(name, env, ride)
        assert health["late_left"] == 0, (arm, health)
        if reaches and "always" in arm:
            assert st["rounds"] > 0 and st["cuts"] > 0, (arm, st)
            if "multi-kernel" in arm:
                assert st["fallback_prunes"] > 0, (arm, st)
        ph.assert_same(ph.canonical(d), exp)


# ---- (c) forced single-cut modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [7, 10, 11, 16])
def test_forced_single_cut_modes_match_oracle_slotwise(q):
    """decline, no_spec, no_hot and the multi-kernel prune (test_poly_modes_gpu.MODES) on the truncated simplex, batch mode 0"""
    name = "truncated simplex q%d" % q
    vals, k0 = CASES[name][1], CASES[name][5]
    rco, do = oracle_run(name)
    n = len(vals) - k0
    assert not any(rco) and n == 2 * (q + 1)              # every cut removes something: each is one pass of the single-cut pipeline
    for mode, env in MODES.items():
        rcg, dg = gpu_run(env, q, vals, k0, 0, 64)
        assert list(rco) == [int(r) for r in rcg], mode
        assert_slotwise_equal(do, dg)
        # the hook drove the run down its path (check_paths of test_poly_modes_gpu, with counts that fit 16 to 34 cuts)
        p = dg["paths"]
        assert p["single_cuts"] >= n and p["hot_chunks"] == 0, (mode, p)
        if "no_spec" in mode:
            assert p["speculative"] == 0, (mode, p)
        elif mode != "decline":
            assert p["speculative"] >= n // 2, (mode, p)
        if mode == "decline":
            assert p["declined"] >= n // 2, (mode, p)          # a corner cut makes more than 3 vertices
        if mode.startswith("multi_kernel_prune"):
            assert p["prune_fallbacks"] >= n // 2, (mode, p)
        if mode == "default":
            assert p["declined"] == 0 and p["prune_fallbacks"] == 0, (mode, p)


# ---- (d) classify_batch against numpy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [7, 9, 10, 11, 13, 16])
def test_classify_batch_matches_numpy(q):
    """test_poly_gpu.test_classify_batch_matches_numpy on the truncated simplex of dimension q: 70 halfspaces, the first ten through
    existing vertices, compared away from the two band edges (numpy has no fma)"""
    vals, k0 = CASES["truncated simplex q%d" % q][1], q + 1
    G = PolyEngine(q)
    ph.run_sequence(G, vals, None, k0)
    d = G.dump()
    rng = np.random.default_rng(3)
    B = 70
    hps = np.hstack([rng.normal(size=(B, q)), -np.abs(rng.normal(size=(B, 1)))])
    live = np.nonzero(d["pu"] & (1 - d["pi"]))[0]
    for k in range(10):
        hps[k, q] = hps[k, :q] @ d["X"][live[k]]
    words, anym, _ = G.classify_batch(hps)
    G.close()
    X, used, ideal = d["X"], d["pu"].astype(bool), d["pi"].astype(bool)
    nsafe = 0
    for b in range(B):
        s = np.zeros(len(X))
        for k in range(q):
            s = s + hps[b, k] * X[:, k]
        a = np.where(ideal, 0.0, hps[b, q])
        cls = np.where(s > a + 1e-9, 3, np.where(s > a - 1e-9, 2, 1))
        cls = np.where(used, cls, 0)
        got = (words[b // 32] >> np.uint64(2 * (b % 32))) & np.uint64(3)
        safe = np.abs(np.abs(s - a) - 1e-9) > 1e-12
        nsafe += int(safe.sum())
        assert np.array_equal(got[safe], cls[safe].astype(np.uint64)), b
        assert anym[b] >= int(np.any(cls[safe] == 1))
        if b < 10:
            assert cls[live[b]] == 2 and got[live[b]] == 2          # the vertex the plane was put through lies on it
    assert nsafe >= 0.95 * B * len(X), nsafe


# ---- (e) bslv_poly_check ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", DIMS)
def test_check_is_clean_on_the_finished_state(q):
    vals, k0 = CASES["truncated simplex q%d" % q][1], q + 1
    G = PolyEngine(q)
    ph.run_sequence(G, vals, None, k0)
    got = G.check()
    G.close()
    print("check", got["out"], "worst", got["worst"])
    assert_clean(got)
    _, do = oracle_run("truncated simplex q%d" % q)
    assert got["out"][0] == int(do["pu"].sum()) and got["out"][6] == len(do["E"]) and got["out"][2] == len(do["I"])


@pytest.mark.parametrize("sign", [1e-3, -1e-3])
def test_check_sees_a_moved_coordinate_at_d16_and_only_it(sign):
    """test_poly_check_gpu.test_each_defect_is_seen_and_only_it at d = 16, on the polytope whose vertices lie on 16 to 20 facets: all
    twelve counts and the offenders are those of the numpy restatement applied to the damaged dump"""
    q, vals, ideals, apex, init_after, k0 = CASES["degenerate simplex q16"]
    G = PolyEngine(q)
    ph.run_sequence(G, vals[:q + 1 + q // 2], None, init_after)          # (the restatement is quadratic: the state before the corner ring)
    assert_clean(G.check())
    d0 = G.dump()
    live = np.nonzero(d0["pu"])[0]
    G.debug_corrupt(3, int(live[2]), q - 1, sign)
    got = assert_matches_restatement(G)
    assert not got["clean"]
    assert got["out"][3] >= 1 and got["out"][4] == 0 and got["worst"][0] > 1e-4
    assert {o[1] for o in got["offenders"] if o[0] in (3, 5)} == {int(live[2])}
    G.close()


# ---- (f) lowerV2upperH and upperV2lowerH ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("v2h", [ph.LOWER2UPPER, ph.UPPER2LOWER])
@pytest.mark.parametrize("q", [7, 11, 16])
def test_upper_and_lower_image_modes_match_oracle_slotwise(q, v2h):
    """the truncated simplex's halfspaces under a projective map that makes them halfspaces of the mode (ph.upper_image_sequence),
    with c = (0.5, 0.75, 1, 0.5, ..., 1): an unbounded polyhedron with vertices and extreme directions"""
    vals, k0 = ph.truncated_simplex(q, 2 * (q + 1), 5)
    c = np.concatenate([0.5 + np.arange(q - 1) % 3 * 0.25, [1.0]])
    V = ph.upper_image_sequence(vals, c, v2h)
    do, dg = run_both(q, V, None, k0, v2h=v2h, c=c)
    assert do["pi"][do["pu"].astype(bool)].sum() >= q and int(do["pu"].sum()) > 20 * q          # directions, and more than a cone
    assert_slotwise_equal(do, dg)
    do, dg = run_both(q, V, None, k0, v2h=v2h, c=c, batched=True, mode=0)
    assert_slotwise_equal(do, dg)


# ---- (g) the argument edge ------------------------------------------------------------------------------------------------------
def test_create_refuses_dimensions_outside_2_to_16():
    import ctypes
    lib = load_library()
    _bind(lib)
    for dim, rc in ((1, 2), (17, 2), (0, 2), (-1, 2)):          # BSLV_E_ARG
        h = ctypes.c_void_p()
        assert lib.bslv_poly_create(ctypes.byref(h), dim, 0, None) == rc, dim
        assert not h.value
    G = PolyEngine(16)
    assert G.lib.bslv_poly_dim(G.h) == 16
    G.close()


# ---- against the compiled reference's results (tests/golden/poly_ref_dims.npz) ----------------------------------------------------
_GOLD = np.load(os.path.join(HERE, "golden", "poly_ref_dims.npz"))
_META = json.load(open(os.path.join(HERE, "golden", "poly_ref_dims.json")))


@pytest.mark.parametrize("name", ["truncated_simplex_q10", "truncated_simplex_q16", "ideal_cone_q16", "degenerate_simplex_q16"])
def test_engine_matches_reference_fixture(name):
    q, v2h, apex, init_after = [int(x) for x in _GOLD[name + "/in_meta"]]
    G = PolyEngine(q, v2h)
    if apex:
        G.dual0_apex()
    rcs = ph.run_sequence(G, _GOLD[name + "/in_vals"], list(_GOLD[name + "/in_ideals"]), None if init_after < 0 else init_after)
    G.dual_adjacency()
    can = ph.canonical(G.dump())
    G.close()
    assert list(rcs) == list(_GOLD[name + "/rc"])
    ph.assert_matches_dims_golden(can, _GOLD, _META, name)
