"""CPU: the library exports the switch for canonical optimal points of objective batches (include/bslv_hip.h,
bslv_lpq_set_canonical_obj, and bslv_vlp_last_canonical_obj_stats of the dual variant), the header declares it and cites where the
reference takes the point of the cut from, the Python mirrors exist, and the case sets of tests/canonical_obj_cases.py meet their
conditions (HiGHS alone: no compute on a device)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_canonical_obj", "bslv_lpq_get_canonical_obj", "bslv_lpq_last_canonical_obj_stats",
       "bslv_vlp_last_canonical_obj_stats"]       # (the fifth new name is the flag BSLV_VLP_CANONICAL: checked in the header)


def test_canonical_obj_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_canonical_obj_symbols_declared_with_their_source():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert re.search(r"\bBSLV_VLP_CANONICAL\s*=\s*4\b", code)
    # the doc comment in front of the switch names the lines the point of the cut comes from
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_lpq_set_canonical_obj")], flags=re.S)[-1]
    assert "bslv_algs.c:1479" in comment
    # ... and the older switch no longer says that objective batches have none
    older = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_lpq_set_canonical(")], flags=re.S)[-1]
    assert "bslv_lpq_set_canonical_obj" in older


def test_python_mirror_has_the_switch():
    import inspect
    from bensolve_amd.lp import LpEngine
    from bensolve_amd import vlp
    assert callable(LpEngine.set_canonical_obj) and callable(LpEngine.get_canonical_obj) and callable(LpEngine.last_canonical_obj_stats)
    assert list(inspect.signature(LpEngine.set_canonical_obj).parameters) == ["self", "on", "cost_first", "ddir"]
    assert inspect.signature(vlp.solve_primal).parameters["canonical"].default is False


@pytest.mark.parametrize("name", ["covering-40x20x4", "covering-30x80x3", "wide-40x1600x3"])
def test_covering_case_sets_meet_their_conditions(name):
    import canonical_obj_cases as co
    prob, c = co.cases(name)
    print("%s: %d of %d kept, %d degenerate, %d facet normals" % (name, len(c["W"]), c["candidates"], int(c["degenerate"].sum()), c["facet_normals"]))
    co.check_case_set(c)
    # every expected y is optimal for its w and a point of the image
    np.testing.assert_allclose(np.einsum("bk,bk->b", c["W"], c["y"]), c["z"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("q", [3, 4])
def test_decoy_case_sets(q):
    import canonical_obj_cases as co
    prob, c = co.cases("decoy-%d" % q)
    V = co.decoy_vertices(q)
    assert prob["n"] == {3: 7, 4: 11}[q]
    assert c["dropped"] == 0 and int(c["degenerate"].sum()) >= 4
    print("decoy-%d: %d weights, %d degenerate" % (q, len(c["W"]), int(c["degenerate"].sum())))
    for y in c["y"]:                              # the canonical point is a vertex of the image, never a decoy
        assert np.abs(V - y).max(axis=1).min() <= 1e-9, y
    if q == 3:
        np.testing.assert_allclose(c["W"][0], np.ones(3) / 3)
        np.testing.assert_allclose(c["y"][0], [2.0, 2.0, 0.0], atol=1e-12)
