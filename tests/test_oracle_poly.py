"""CPU: the oracle polyhedron restatement (oracle/poly_dd.c) against golden outputs of the REFERENCE
polyhedron engine (tests/golden/poly_ref.npz, made by make_golden.py from the unmodified
bslv_poly.c) and, where oracle/_ref exists, against the compiled reference live as well."""
import os
import numpy as np
import pytest

import poly_harness as ph

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "poly_ref.npz"))
NAMES = sorted({k.split("/")[0] for k in GOLD.files})


def golden_case(name):
    q, v2h, apex, init_after = [int(x) for x in GOLD[name + "/in_meta"]]
    return q, v2h, bool(apex), (None if init_after < 0 else init_after), GOLD[name + "/in_vals"], GOLD[name + "/in_ideals"]


def golden_canonical(name):
    g = lambda k: GOLD[name + "/" + k]
    return dict(X=g("X"), pi=g("pi"), Y=g("Y"), di=g("di"), E={tuple(e) for e in g("E")}, I={tuple(e) for e in g("I")},
                DE={tuple(e) for e in g("DE")})


def run_engine(P, name):
    q, v2h, apex, init_after, vals, ideals = golden_case(name)
    if apex:
        P.dual0_apex()
    rcs = ph.run_sequence(P, vals, list(ideals), init_after)
    P.dual_adjacency()
    return rcs, ph.canonical(P.dump())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_golden(name):
    q, v2h, apex, init_after, vals, ideals = golden_case(name)
    P = ph.FlatPoly("oracle", q, v2h)
    rcs, can = run_engine(P, name)
    P.close()
    assert list(rcs) == list(GOLD[name + "/rc"])            # same cuts found redundant (EXIT_FAILURE)
    ph.assert_same(can, golden_canonical(name))


import json
GOLD_L = np.load(os.path.join(HERE, "golden", "poly_ref_large.npz"))
META_L = json.load(open(os.path.join(HERE, "golden", "poly_ref_large.json")))


@pytest.mark.parametrize("name", sorted(META_L))
def test_oracle_matches_reference_golden_at_survey_sizes(name):
    """SURVEY.md 8c's sizes (q=3 N=2000, q=5 N=200 / N=1000, q=8 N=60, ex06's dual cone, ex10's lattice directions): the
    reference's own bslv_poly.c produced the fixture (tests/golden/make_golden.py large); coordinates at 1e-9, index sets
    bit-exact by SHA-256 of the canonical labelling"""
    q, v2h, apex, init_after = [int(x) for x in GOLD_L[name + "/in_meta"]]
    P = ph.FlatPoly("oracle", q, v2h)
    if apex:
        P.dual0_apex()
    rcs = ph.run_sequence(P, GOLD_L[name + "/in_vals"], list(GOLD_L[name + "/in_ideals"]), None if init_after < 0 else init_after)
    P.dual_adjacency()
    can = ph.canonical(P.dump())
    P.close()
    assert list(rcs) == list(GOLD_L[name + "/rc"])
    ph.assert_matches_large_golden(can, GOLD_L, META_L, name)


GOLD_D = np.load(os.path.join(HERE, "golden", "poly_ref_dims.npz"))
META_D = json.load(open(os.path.join(HERE, "golden", "poly_ref_dims.json")))
NAMES_D = sorted({k.split("/")[0] for k in GOLD_D.files})


def test_dims_fixture_holds_the_cases_of_the_generators():
    """the inputs stored with the fixture are what poly_harness's generators give today, so the GPU tests (which call the generators)
    and this file (which reads the fixture) speak of the same polyhedra; and the file stays below poly_ref.npz"""
    exp = {}
    for q in (7, 9, 10, 11, 12, 16):
        exp["truncated_simplex_q%d" % q] = ph.truncated_simplex(q, 2 * (q + 1), 5)
    for q in (7, 8):
        exp["cross_q%d" % q] = (ph.sign_vectors(q), -1)
    exp["cube_trunc_q7"] = (ph.truncated_cube(7), -1)
    for q in (7, 11, 16):
        exp["ideal_cone_q%d" % q] = (ph.ideal_cone(q, 3), -1)
    for q in (11, 16):
        exp["degenerate_simplex_q%d" % q] = ph.degenerate_simplex(q, 0)
    assert sorted(exp) == NAMES_D
    for name, (vals, k0) in exp.items():
        assert np.array_equal(GOLD_D[name + "/in_vals"], vals), name
        assert int(GOLD_D[name + "/in_meta"][3]) == k0 and int(GOLD_D[name + "/in_meta"][0]) == vals.shape[1], name
    size = lambda f: os.path.getsize(os.path.join(HERE, "golden", f))
    assert size("poly_ref_dims.npz") < size("poly_ref.npz")


@pytest.mark.parametrize("name", NAMES_D)
def test_oracle_matches_reference_golden_at_dimensions_7_to_16(name):
    """dimensions the other fixtures do not reach (7, 9, 10, 11, 12, 16; tests/golden/make_golden.py dims, from the unmodified
    bslv_poly.c): the same cuts found redundant, the same canonical sets, coordinates at 1e-9.  Where oracle/_ref exists the compiled
    reference runs live through the same comparison."""
    q, v2h, apex, init_after = [int(x) for x in GOLD_D[name + "/in_meta"]]
    for kind in ("oracle", "ref") if ph.ref_available() else ("oracle",):
        P = ph.FlatPoly(kind, q, v2h)
        if apex:
            P.dual0_apex()
        rcs = ph.run_sequence(P, GOLD_D[name + "/in_vals"], list(GOLD_D[name + "/in_ideals"]), None if init_after < 0 else init_after)
        P.dual_adjacency()
        can = ph.canonical(P.dump())
        P.close()
        assert list(rcs) == list(GOLD_D[name + "/rc"]), kind
        ph.assert_matches_dims_golden(can, GOLD_D, META_D, name)


@pytest.mark.parametrize("v2h", [ph.LOWER2UPPER, ph.UPPER2LOWER])
@pytest.mark.parametrize("q", [7, 11, 16])
def test_oracle_matches_compiled_reference_in_the_image_modes(q, v2h):
    """lowerV2upperH / upperV2lowerH with a non-trivial c at d = 7, 11, 16 (the sequences of tests/test_poly_dims_gpu.py): no fixture
    carries c, so this comparison runs where the compiled reference exists; without it the oracle's result is checked for what the
    map promises -- every live vertex satisfies every applied halfspace of the mode and lies on those it lists"""
    vals, k0 = ph.truncated_simplex(q, 2 * (q + 1), 5)
    c = np.concatenate([0.5 + np.arange(q - 1) % 3 * 0.25, [1.0]])
    V = ph.upper_image_sequence(vals, c, v2h)
    res = {}
    for kind in ("oracle", "ref") if ph.ref_available() else ("oracle",):
        P = ph.FlatPoly(kind, q, v2h, c)
        rcs = ph.run_sequence(P, V, None, k0)
        P.dual_adjacency()
        res[kind] = (list(rcs), P.dump())
        P.close()
    if "ref" in res:
        assert res["oracle"][0] == res["ref"][0]
        ph.assert_same(ph.canonical(res["oracle"][1]), ph.canonical(res["ref"][1]))
    d = res["oracle"][1]
    if v2h == ph.LOWER2UPPER:
        H = np.hstack([V[:, :q - 1], 1.0 - V[:, :q - 1] @ c[:q - 1, None], V[:, q - 1:]])
    else:
        H = np.hstack([V[:, :q - 1] - V[:, q - 1:] * c[None, :q - 1], -np.ones((len(V), 1)), -V[:, q - 1:]])
    pts = d["pu"].astype(bool) & (d["pi"] == 0)
    dirs = d["pu"].astype(bool) & (d["pi"] == 1)
    assert pts.sum() > 10 * q and dirs.sum() >= q
    assert (d["X"][pts] @ H[:, :q].T - H[:, q][None, :]).min() > -1e-9 * (1 + np.abs(d["X"][pts]).max())
    assert (d["X"][dirs] @ H[:, :q].T).min() > -1e-9
    # a listed incidence is geometric: dual slot f >= 1 holds input f - 1 until the start re-adds the cuts it did not choose
    Yall = d["Y"]
    if v2h == ph.LOWER2UPPER:
        Hall = np.hstack([Yall[:, :q - 1], 1.0 - Yall[:, :q - 1] @ c[:q - 1, None], Yall[:, q - 1:]])
    else:
        Hall = np.hstack([Yall[:, :q - 1] - Yall[:, q - 1:] * c[None, :q - 1], -np.ones((len(Yall), 1)), -Yall[:, q - 1:]])
    I = d["I"][pts[d["I"][:, 0]] & (d["di"][d["I"][:, 1]] == 0)]
    res_inc = np.einsum("ij,ij->i", d["X"][I[:, 0]], Hall[I[:, 1], :q]) - Hall[I[:, 1], q]
    assert np.abs(res_inc).max() < 1e-9 * (1 + np.abs(d["X"][pts]).max())


GOLD_LIVE = np.load(os.path.join(HERE, "golden", "poly_ref_live.npz"))


@pytest.mark.parametrize("q,N,seed", [(3, 500, 21), (4, 150, 22), (5, 150, 23)])
def test_oracle_matches_compiled_reference_live(q, N, seed):
    """against the reference's result for the same sequence: stored in tests/golden/poly_ref_live.npz (make_golden.py live), and
    where oracle/_ref exists also the compiled reference run live"""
    D = ph.tangent_halfspaces(q, N, seed)
    kinds = ("oracle", "ref") if ph.ref_available() else ("oracle",)
    res = {}
    for kind in kinds:
        P = ph.FlatPoly(kind, q)
        ph.run_sequence(P, D, init_after=q + 2)
        P.dual_adjacency()
        res[kind] = ph.canonical(P.dump())
        P.close()
    g = lambda k: GOLD_LIVE["tangent_q%d_N%d_s%d/%s" % (q, N, seed, k)]
    gold = dict(X=g("X"), pi=g("pi"), Y=g("Y"), di=g("di"), E={tuple(e) for e in g("E")}, I={tuple(e) for e in g("I")},
                DE={tuple(e) for e in g("DE")})
    for kind in kinds:
        ph.assert_same(res[kind], gold)


def test_get_vrtx_order_and_marks():
    # poly__get_vrtx returns the lowest live slot without the sltn mark (bslv_poly.c:210-226)
    P = ph.FlatPoly("oracle", 3)
    ph.run_sequence(P, ph.tangent_halfspaces(3, 20, 5))
    seen = []
    while True:
        nxt = P.next()
        if nxt is None:
            break
        seen.append(nxt[2])
        P.mark(nxt[2])
    d = P.dump()
    assert seen == sorted(seen) and len(seen) == int(d["pu"].sum())
    P.close()


GOLD_S = np.load(os.path.join(HERE, "golden", "poly_ref_snap.npz"))


def run_snap_case(name, snap):
    import ctypes
    q, v2h, apex, init_after = [int(x) for x in GOLD_S[name + "/in_meta"]]
    P = ph.FlatPoly("oracle", q, v2h)
    P.L.opoly_set_snap.argtypes = [ctypes.c_void_p, ctypes.c_int]
    P.L.opoly_snapped.argtypes = [ctypes.c_void_p]
    P.L.opoly_snapped.restype = ctypes.c_long
    P.L.opoly_set_snap(P.h, snap)
    rcs = ph.run_sequence(P, GOLD_S[name + "/in_vals"], list(GOLD_S[name + "/in_ideals"]), init_after)
    P.dual_adjacency()
    can, moved = ph.canonical(P.dump()), P.L.opoly_snapped(P.h)
    P.close()
    g = lambda k: GOLD_S[name + "/" + k]
    gold = dict(X=g("X"), pi=g("pi"), Y=g("Y"), di=g("di"), E={tuple(e) for e in g("E")}, I={tuple(e) for e in g("I")}, DE={tuple(e) for e in g("DE")})
    assert list(rcs) == list(g("rc"))
    return can, gold, moved


@pytest.mark.parametrize("name", sorted({k.split("/")[0] for k in GOLD_S.files}))
def test_snap_band_of_poly_cut_against_the_reference(name):
    """bslv_poly.c:666-674: a neighbour of a removed element that lies between 1e-2 POLY_EPS and POLY_EPS above the cut is moved ONTO the
    hyperplane before it is treated as lying on it.  Fixtures (tests/golden/make_golden.py snap, from the unmodified bslv_poly.c): one
    crafted cut passes delta above a live vertex, twelve ordinary cuts follow.  With opoly_set_snap(1) the oracle restates the band and
    agrees with the reference to 1e-13 -- for delta inside the band (5e-10, 5e-11: one element moved) and below it (5e-12: none moved).
    With the switch off -- the default of the oracle and of the HIP engine (bslv_poly_set_snap) -- the index sets are the
    same and the coordinates differ by less than 1e-9, i.e. invisibly at the tolerance of every other comparison with the reference,
    but by more than 1e-11 where the band is hit: the size of the gap, measured."""
    delta = float(name.split("delta")[1])
    can, gold, moved = run_snap_case(name, 1)
    ph.assert_same(can, gold, rtol=0, atol=1e-13)
    assert moved == (1 if delta > 1e-11 else 0)
    can0, gold, moved0 = run_snap_case(name, 0)
    assert moved0 == 0
    ph.assert_same(can0, gold, rtol=0, atol=1e-9)
    gap = np.abs(can0["X"] - gold["X"]).max()
    if delta > 1e-11:
        assert 1e-11 < gap < 1e-9, gap
    else:
        assert gap < 1e-13, gap


GOLD_SD = np.load(os.path.join(HERE, "golden", "poly_ref_snap_dirs.npz"))


@pytest.mark.parametrize("name", sorted({k.split("/")[0] for k in GOLD_SD.files}))
def test_snap_band_moves_directions_too(name):
    """The same band for an ideal element (alpha = 0 in poly__cut's comparisons, bslv_poly.c:596,666): an unbounded polyhedron, a cut
    crafted so that w.r = delta for one of its extreme directions r while a neighbour of r is removed, eight ordinary cuts behind it
    (tests/golden/make_golden.py snap, from the unmodified bslv_poly.c).  The polyhedron has vertices with coordinates of ~6 next to the
    moved direction, where the reference's plain sums and the oracle's fma chains differ in the last bits: 1e-12 here, not 1e-13.
    The engine runs the same fixture in tests/test_poly_gpu.py::test_snap_band_moves_a_direction_as_the_reference_does."""
    import ctypes
    delta = float(name.split("delta")[1])
    q, v2h, apex, init_after = [int(x) for x in GOLD_SD[name + "/in_meta"]]
    g = lambda k: GOLD_SD[name + "/" + k]
    gold = dict(X=g("X"), pi=g("pi"), Y=g("Y"), di=g("di"), E={tuple(e) for e in g("E")}, I={tuple(e) for e in g("I")}, DE={tuple(e) for e in g("DE")})
    gaps = {}
    for snap in (1, 0):
        P = ph.FlatPoly("oracle", q, v2h)
        P.L.opoly_set_snap.argtypes = [ctypes.c_void_p, ctypes.c_int]
        P.L.opoly_snapped.argtypes = [ctypes.c_void_p]
        P.L.opoly_snapped.restype = ctypes.c_long
        P.L.opoly_set_snap(P.h, snap)
        rcs = ph.run_sequence(P, g("in_vals"), list(g("in_ideals")), init_after)
        P.dual_adjacency()
        can, moved = ph.canonical(P.dump()), P.L.opoly_snapped(P.h)
        P.close()
        assert list(rcs) == list(g("rc"))
        assert moved == (1 if snap and delta > 1e-11 else 0)
        ph.assert_same(can, gold, rtol=1e-12 if snap else 1e-8, atol=1e-12 if snap else 1e-8)
        gaps[snap] = (np.abs(can["X"] - gold["X"]) / (1.0 + np.abs(gold["X"]))).max()        # (far vertices of an unbounded polyhedron: relative)
    if delta > 1e-11:
        assert gaps[0] > 10 * gaps[1] and gaps[0] > 1e-11, gaps
