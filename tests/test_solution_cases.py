"""CPU: the general cases of tests/vlp_general_cases.py and their goldens (tests/golden/solutions.npz / .json, written by
`tests/golden/make_golden.py solutions` from the hybrid's -s runs) meet the conditions tests/test_solutions_gpu.py relies on.
Runs from the goldens alone; where oracle/_ref/bensolve_hybrid exists the hybrid runs again and must reproduce them."""
import json
import os
import sys

import numpy as np
import pytest

import solution_certificate as sc
import vlp_general_cases as gc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "solutions.npz"))
META = json.load(open(os.path.join(HERE, "golden", "solutions.json")))
HYB = os.path.join(ROOT, "oracle", "_ref", "bensolve_hybrid")
RUNS = [(name + sfx, name) for name in gc.CASES for sfx in (("", "+b") if name in gc.BOUNDED else ("",))]


def test_every_run_has_a_golden():
    assert sorted(META) == sorted(k for k, _ in RUNS)
    assert sorted({k.split("/")[0] for k in GOLD.files}) == sorted(META)


@pytest.mark.parametrize("key,name", RUNS)
def test_case_conditions(key, name):
    prob, meta = gc.CASES[name](), META[key]
    assert gc.digest(prob) == meta["digest"]                         # the goldens belong to these inputs
    assert meta["rc"] == 0
    assert meta["points"] >= 6 and meta["dual_vertices"] >= 6
    assert len(GOLD[key + "/p"]) == meta["points"] + meta["directions"] and len(GOLD[key + "/d"]) == meta["dual_vertices"] + meta["dual_directions"]
    assert GOLD[key + "/c"].shape == (prob["q"],)
    # separation: the sorted comparison of tests/test_solutions_gpu.py is stable
    for side in ("p", "d"):
        Z = GOLD[key + "/" + side][GOLD[key + "/" + side + "_type"] == 1]
        gap = min(np.abs(Z[i] - Z[j]).max() for i in range(len(Z)) for j in range(i))
        assert gap >= 1e-4, (side, gap)
    if name.startswith("U"):
        assert meta["directions_outside_cone"] >= 1
    assert meta["singleton_rows"] == len(gc.singleton_rows(prob))
    if meta["singleton_rows"]:
        assert meta["max_abs_u_on_singleton_rows"] > 1e-3
    # the reference's own files pass the certificate, apart from at most one dual vertex whose (u, w) belongs to another one
    assert len(meta["w_mismatch"]) <= 1
    for k in sc.CHECKS:
        assert meta["residuals"][k]["value"] <= sc.REF_BOUND * meta["scale"], (k, meta["residuals"][k])


def test_the_reference_fails_its_own_w_check_somewhere():
    """what the GPU test holds the product to and the reference does not meet: keep at least one such case among the goldens"""
    assert sorted(k for k, v in META.items() if v["w_mismatch"]) == ["B3max-cone", "B3max-cone+b", "U3-cone", "U3max", "U4"]


@pytest.mark.skipif(not os.path.exists(HYB), reason="the hybrid is built only where the reference's sources are")
@pytest.mark.parametrize("key,name", RUNS)
def test_hybrid_reproduces_the_goldens(key, name):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden
    prob = gc.CASES[name]()
    rc, run = make_golden.run_hybrid_solution(prob, ["-b"] if key.endswith("+b") else [])
    assert rc == META[key]["rc"] == 0
    for side in ("p", "d"):
        t, X, _ = sc.sorted_img(run["img_" + side])
        gt, gX, _ = sc.sorted_img(np.column_stack([GOLD[key + "/" + side + "_type"], GOLD[key + "/" + side]]))
        assert np.array_equal(t, gt)
        np.testing.assert_allclose(X, gX, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(run["c"], GOLD[key + "/c"], rtol=0, atol=1e-12)
    rec = sc.reference_record(prob, run)
    assert rec["w_mismatch"] == META[key]["w_mismatch"]
    for k in ("points", "directions", "directions_outside_cone", "dual_vertices", "dual_directions"):
        assert rec[k] == META[key][k], k
    for k in sc.CHECKS:
        assert rec["residuals"][k]["value"] <= sc.REF_BOUND * rec["scale"], (k, rec["residuals"][k])


# ---- the certificate itself: it must see what it is there to see ----
def _golden_like_run():
    """a consistent set of files made by hand for a 2-objective problem:  min (x1, x2)  s.t.  x1 + x2 >= 1 (row 'l'), 2 x1 <= 4 (a
    singleton 'u' row), x >= 0.  Upper image: vertices (1, 0), (0, 1), directions e1, e2.  Lower image vertices y* = (w1, u . b)."""
    prob = dict(m=2, n=2, q=2, optdir=1, A=np.array([[1.0, 1.0], [2.0, 0.0]]), P=np.eye(2), rtype=np.frombuffer(b"lu", np.uint8), rlb=np.array([1.0, 0.0]),
                rub=np.array([0.0, 4.0]), ctype=np.frombuffer(b"ll", np.uint8), clb=np.zeros(2), cub=np.zeros(2))
    run = dict(img_p=np.array([[1, 1.0, 0.0], [1, 0.0, 1.0], [0, 1.0, 0.0], [0, 0.0, 1.0]]), pre_p=np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]),
               img_d=np.array([[1, 0.0, 0.0], [1, 0.5, 0.5], [1, 1.0, 0.0], [0, 0.0, -1.0]]),
               pre_d=np.array([[0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.5, 0.5], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]), c=np.ones(2))
    return prob, run


def test_certificate_accepts_a_hand_made_solution():
    prob, run = _golden_like_run()
    res = sc.certify(prob, run, 1e-7)
    for k in sc.CHECKS:
        assert res[k]["value"] <= 1e-15, (k, res[k])


@pytest.mark.parametrize("what,check", [("u_sign", "dual_sign_u"), ("u_row_swap", "dual_objective"), ("w_other_vertex", "dual_w_of_vertex"), ("x_infeasible", "point_rows"),
                                         ("x_column", "point_columns"), ("x_other_vertex", "point_image"), ("y_inside", "duality_outer"), ("y_outside", "duality_eps"),
                                         ("w_outside_cone", "dual_w_in_cone"), ("dir_x_not_recession", "direction_rows"), ("dir_outside_cone_with_x_0", "direction_image"),
                                         ("d_sign", "dual_sign_d"), ("point_not_dominating", "point_domination")])
def test_certificate_sees_a_wrong_file(what, check):
    prob, run = _golden_like_run()
    run = {k: v.copy() for k, v in run.items()}
    if what == "u_sign":
        run["pre_d"][1, 0] = -0.5
    elif what == "u_row_swap":
        run["pre_d"][1, :2] = [0.0, 0.5]
    elif what == "w_other_vertex":
        run["pre_d"][1, 2:] = [1.0, 0.0]
    elif what == "x_infeasible":
        run["pre_p"][0] = [0.5, 0.0]
    elif what == "x_column":
        run["pre_p"][0] = [1.5, -0.5]
    elif what == "x_other_vertex":
        run["pre_p"][0] = [0.0, 1.0]
    elif what == "y_inside":
        run["img_p"][0, 1:] = [0.4, 0.4]; run["pre_p"][0] = [0.4, 0.6]
    elif what == "y_outside":
        run["img_p"][0, 1:] = [1.5, 0.5]; run["pre_p"][0] = [1.5, 0.5]
    elif what == "w_outside_cone":
        run["pre_d"][2, 2:] = [1.25, -0.25]
    elif what == "dir_x_not_recession":
        run["pre_p"][2] = [1.0, -1.0]
    elif what == "dir_outside_cone_with_x_0":
        run["img_p"][2, 1:] = [1.0, -0.5]
    elif what == "d_sign":
        run["pre_d"][1, :2] = [1.0, 0.0]                                  # A'u = (1, 1) > P'w = (0.5, 0.5) on columns without an upper bound
    elif what == "point_not_dominating":
        run["img_p"][0, 1:] = [1.0, -0.25]                               # x = (1, 0) gives P x = (1, 0), which does not lie below y
    res = sc.certify(prob, run, 1e-7)
    assert res[check]["value"] > 1e-3, (check, res[check])


def test_dual_rays_of_the_cones_in_use():
    for name in ("B3max-cone", "U3-cone", "U2-dualcone"):
        prob = gc.CASES[name]()
        gC, gCp = sc.cone_generators(prob)
        assert len(gC) >= prob["q"] and len(gCp) >= prob["q"]
        assert (gC @ gCp.T).min() >= -1e-12
        # every generator of one cone lies on q - 1 facets of it, i.e. is orthogonal to at least q - 1 generators of the other
        for a, b in ((gC, gCp), (gCp, gC)):
            found = sc.dual_rays(a.T)
            assert len(found) and all((np.abs(f @ a.T) < 1e-9).sum() >= prob["q"] - 1 for f in found)
