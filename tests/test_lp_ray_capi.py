"""CPU: the ray store and its certificate at the ABI -- the header declares bslv_lpq_set_rays / get_rays / get_ray / last_ray_stats /
certify_rays / last_ray_certify_stats and the three kinds, the library exports them, the Python mirrors exist, calls with a null engine
are refused -- and the yardstick of the GPU tests (tests/lp_ray_cases.py) on hand-made cases and on every boxed set: the inputs are what
the GPU tests take them for before anything goes to the GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lp_ray_cases as rc
from lp_ray_cases import FARKAS, DIRECTION, NONE

NEW = ["bslv_lpq_set_rays", "bslv_lpq_get_rays", "bslv_lpq_get_ray", "bslv_lpq_last_ray_stats", "bslv_lpq_certify_rays", "bslv_lpq_last_ray_certify_stats"]


def _header():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_ray_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_ray_symbols_declared():
    txt, code = _header()
    flat = re.sub(r"\s+", " ", code)
    assert "enum { BSLV_LP_RAY_NONE = 0, BSLV_LP_RAY_FARKAS = 1, BSLV_LP_RAY_DIRECTION = 2 };" in flat
    assert "int bslv_lpq_set_rays(bslv_lpq *h, int on);" in flat
    assert "int bslv_lpq_get_rays(const bslv_lpq *h);" in flat
    assert "int bslv_lpq_get_ray(bslv_lpq *h, int B, const int *slot, int *kind , double *ray );" in flat
    assert "int bslv_lpq_last_ray_stats(const bslv_lpq *h, long out[3]);" in flat
    assert ("int bslv_lpq_certify_rays(bslv_lpq *h, int B, const int *slot, const double *vlo, const double *vup, int cost_first, int cost_cnt, "
            "const double *costs, const double *tol , double *res , int *at , int *verdict );") in flat
    assert "int bslv_lpq_last_ray_certify_stats(const bslv_lpq *h, long out[3]);" in flat
    # the contract in front of the store: the three conclusions, the two that store nothing and what a caller does about the first
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("enum { BSLV_LP_RAY_NONE")], flags=re.S)[-1]
    for word in ["BSLV_LP_RAYS=1", "FARKAS, dual row", "FARKAS, phase 1", "DIRECTION", "largest absolute entry", "artificial bound", "a single column is in general not a ray",
                 "BSLV_LP_METHOD_PRIMAL", "empty box", "model AS GIVEN", "z_i = z_j / a_ij", "BSLV_E_STATE", "bslv_lpq_slot_bytes", "bslv_lpq_reset_slot"]:
        assert word in comment, word
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int bslv_lpq_certify_rays(")], flags=re.S)[-1]
    for word in ["Read-only", "ident", "open", "margin", "rows", "cross", "1e-8, 1e-9, 1e-9, 1e-9", "bit 3", "tol[3] (1 + res[3])"]:
        assert word in comment, word


def test_refused_without_a_device():
    from bensolve_amd import load_library
    lib = load_library()
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.bslv_lpq_set_rays.argtypes = [vp, i]
    lib.bslv_lpq_get_rays.argtypes = [vp]
    lib.bslv_lpq_get_ray.argtypes = [vp, i, vp, vp, vp]
    lib.bslv_lpq_last_ray_stats.argtypes = [vp, vp]
    lib.bslv_lpq_certify_rays.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp]
    lib.bslv_lpq_last_ray_certify_stats.argtypes = [vp, vp]
    slot, kind, res = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), (ctypes.c_double * 4)()
    assert lib.bslv_lpq_set_rays(None, 1) == 2          # BSLV_E_ARG
    assert b"bslv_lpq_set_rays" in lib.bslv_last_error()
    assert lib.bslv_lpq_get_rays(None) == 0
    assert lib.bslv_lpq_get_ray(None, 1, slot, kind, None) == 2
    assert b"bslv_lpq_get_ray" in lib.bslv_last_error()
    assert lib.bslv_lpq_last_ray_stats(None, None) == 2
    assert lib.bslv_lpq_certify_rays(None, 1, slot, None, None, 0, 0, None, None, res, None, None) == 2
    assert b"bslv_lpq_certify_rays" in lib.bslv_last_error()
    assert lib.bslv_lpq_last_ray_certify_stats(None, None) == 2


def test_python_mirror_and_sources():
    from bensolve_amd.lp import LpEngine
    for name in ("set_rays", "get_rays", "get_ray", "certify_rays", "last_ray_stats", "last_ray_certify_stats"):
        assert callable(getattr(LpEngine, name)), name
    src = lambda *p: open(os.path.join(ROOT, "bensolve_amd", "csrc", *p)).read()
    eng, inc = src("lp_engine.hip"), src("lp_certify.inc")
    assert "void k_ray(" in eng and "BSLV_LP_RAYS" in eng
    assert "void k_cert_ray_final(" in inc
    assert "atomicAdd" not in inc          # (fixed summation order: no atomics in the arithmetic)
    for f in ("benson_driver.hip", "vlp_phases.hip"):
        assert "report_ray(" in src(f), f


def test_yardstick_on_hand_made_cases():
    A, lo, up, cost = rc.handmade()
    z = np.array([1.0, -1.0, -1.0])
    c = rc.certify_ray(A, lo, up, cost, FARKAS, z)
    assert c["verdict"] == 0 and list(c["res"]) == [0.0, 0.0, 1.0, 5.0] and list(c["at"][1:]) == [-1, -1, -1], c          # S = 3 - 1 - 1, sum |z bound| = 3 + 1 + 1
    A2, lo2, up2, _ = rc.handmade(up2=np.inf)                  # x2 has no upper bound: the entry on it is open
    c = rc.certify_ray(A2, lo2, up2, cost, FARKAS, z)
    assert c["verdict"] & 2 and c["res"][1] == 1.0 and c["at"][1] == 2, c
    c = rc.certify_ray(A, lo, up, cost, FARKAS, np.array([1.0, -1.0, -0.5]))          # not in the row space: z . (A x, x) != 0
    assert c["verdict"] & 1 and c["res"][0] == 0.5 and c["at"][0] == 2, c
    c = rc.certify_ray(A, lo, up, cost, FARKAS, -z)            # the other sign needs the row's upper bound: open
    assert c["verdict"] & 2, c
    c = rc.certify_ray(A, lo, up, cost, NONE, z)
    assert c["verdict"] & 8 and np.isnan(c["res"]).all() and (c["at"] == -1).all(), c
    # a direction: min x1 with x1 free and no row on it
    A = np.array([[0.0, 1.0]])
    lo, up = np.array([0.0, -np.inf, 0.0]), np.array([1.0, np.inf, 1.0])
    cost = np.array([0.0, 1.0, 0.0])
    c = rc.certify_ray(A, lo, up, cost, DIRECTION, np.array([0.0, -1.0, 0.0]))
    assert c["verdict"] == 0 and list(c["res"]) == [0.0, 0.0, 1.0, 1.0], c
    c = rc.certify_ray(A, lo, up, cost, DIRECTION, np.array([0.0, 1.0, 0.0]))          # uphill
    assert c["verdict"] == 4, c
    c = rc.certify_ray(A, lo, up, cost, DIRECTION, np.array([0.0, -1.0, 1.0]))         # x2 leaves its box and the row does not follow
    assert c["verdict"] == 3 and c["res"][0] == 1.0 and c["res"][1] == 1.0 and list(c["at"][:2]) == [0, 2], c


@pytest.mark.parametrize("M,N", rc.SHAPES)
def test_boxed_sets_are_what_the_gpu_tests_take_them_for(oracle, M, N):
    st = rc.assert_boxed_references(M, N)
    assert int(np.sum(st == rc.OPTIMAL)) == 13 and [t for t in range(rc.NLP) if st[t] == rc.INFEASIBLE] == list(rc.BAD_LPS)
    s = rc.boxed_set(M, N)
    # every column boxed and no row folded by the presolve (each row of the per-LP range stays a row)
    assert np.isfinite(s["lo"][M:]).all() and np.isfinite(s["up"][M:]).all()
