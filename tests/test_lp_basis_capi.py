"""CPU: the library exports the calls that take a basis out of a slot and put one in (include/bslv_hip.h: bslv_lpq_var_map,
bslv_lpq_get_basis, bslv_lpq_load_basis, bslv_lpq_rebuild, bslv_lpq_last_rebuild_stats), the header declares them with GLPK's status
codes, LpEngine mirrors them -- and the generator of the bases the GPU tests load (tests/lp_basis_cases.py) is what it says it is."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lp_cases as lc
import lp_basis_cases as bc

NEW = ["bslv_lpq_var_map", "bslv_lpq_get_basis", "bslv_lpq_load_basis", "bslv_lpq_rebuild", "bslv_lpq_last_rebuild_stats"]


def test_basis_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_basis_symbols_declared_with_glpk_codes():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    for name, val in (("BASIC", 1), ("LOWER", 2), ("UPPER", 3), ("FREE", 4), ("FIXED", 5)):       # GLP_BS, GLP_NL, GLP_NU, GLP_NF, GLP_NS
        assert re.search(r"\bBSLV_LP_VS_%s\s*=\s*%d\b" % (name, val), code), name
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("enum { BSLV_LP_VS_BASIC")], flags=re.S)[-1]
    # the comment says what a later solve makes of an infeasible basis under each method, and what a singular basis is
    for word in ("FEASIBILITY IS NOT CHECKED", "BSLV_LP_METHOD_DUAL", "PRIMAL", "REPAIR", "SINGULAR", "bslv_lpq_reset_slot", "artificial"):
        assert word in comment, word


def test_python_mirror_has_the_methods_and_the_codes():
    from bensolve_amd.lp import LpEngine
    for name in ("var_map", "get_basis", "load_basis", "rebuild", "last_rebuild_stats"):
        assert callable(getattr(LpEngine, name)), name
    assert (LpEngine.VS_BASIC, LpEngine.VS_LOWER, LpEngine.VS_UPPER, LpEngine.VS_FREE, LpEngine.VS_FIXED) == (1, 2, 3, 4, 5)
    assert (bc.BASIC, bc.LOWER, bc.UPPER, bc.FREE, bc.FIXED) == (1, 2, 3, 4, 5)


def test_entry_points_refuse_a_missing_engine():
    """no device needed: every new entry point checks its handle first"""
    from bensolve_amd import load_library
    lib = load_library()
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.bslv_lpq_var_map.argtypes = [vp, vp]
    lib.bslv_lpq_get_basis.argtypes = [vp, i, vp, vp]
    lib.bslv_lpq_load_basis.argtypes = [vp, i, vp, vp, vp, vp, vp]
    lib.bslv_lpq_rebuild.argtypes = [vp, i, vp, vp]
    lib.bslv_lpq_last_rebuild_stats.argtypes = [vp, vp]
    out = (ctypes.c_int * 4)()
    assert lib.bslv_lpq_var_map(None, out) == 2          # BSLV_E_ARG
    assert lib.bslv_lpq_get_basis(None, 0, out, None) == 2
    assert lib.bslv_lpq_load_basis(None, 0, None, None, None, None, None) == 2
    assert lib.bslv_lpq_rebuild(None, 0, None, None) == 2
    assert lib.bslv_lpq_last_rebuild_stats(None, None) == 2


def test_the_generator_is_seeded_and_keeps_well_conditioned_bases_only():
    A, lo, up, cost = bc.shape_model(16, 17)
    one = bc.bases(("capi", 1), A, lo, up, cost, 5)
    two = bc.bases(("capi", 2), A, lo, up, cost, 5)
    assert [ns for ns, _, _ in one] == [0, 1, 5, 6, 7, 13, 16] == bc.counts(16, 17)
    for (ns, v1, r1), (_, v2, r2) in zip(one, two):
        assert np.array_equal(v1, v2)
        assert int(np.sum(v1 == bc.BASIC)) == 16 and int(np.sum(v1[16:] == bc.BASIC)) == ns
        s64 = bc.solve_basis(A, lo, up, cost, v1, np.float64)
        for a, b in zip(s64, r1):
            a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
            assert np.max(np.abs(a - b)) <= bc.AGREE * (1.0 + np.max(np.abs(b)))
        # every nonbasic variable rests on a bound it has
        x = bc.nonbasic_values(v1, lo, up)
        assert np.all(np.isfinite(x))


def test_the_host_solution_of_a_basis_is_a_solution():
    A, lo, up, cost = bc.small_model()
    M, N = A.shape
    for ns, vstat, (z, d, obj) in bc.bases("capi-small", A, lo, up, cost, 7):
        z, d = np.asarray(z, np.float64), np.asarray(d, np.float64)
        np.testing.assert_allclose(z[:M], A @ z[M:], atol=1e-12)
        non = vstat != bc.BASIC
        np.testing.assert_array_equal(z[non], bc.nonbasic_values(vstat, lo, up)[non])
        # d = c - A' lambda with lambda = the duals of the rows: the identity the certificate checks (lp_cases.certify, "dj")
        np.testing.assert_allclose(d[M:], cost[1:] - A.T @ d[:M], atol=1e-12)
        assert np.all(d[vstat == bc.BASIC] == 0.0)
        np.testing.assert_allclose(float(obj), cost[0] + cost[1:] @ z[M:], atol=1e-12)
    # the standard basis: the reduced costs are the costs
    std = np.concatenate([np.full(M, bc.BASIC), bc.nonbasic_codes(lo[M:], up[M:], np.random.default_rng(0))]).astype(np.int32)
    z, d, obj = bc.solve_basis(A, lo, up, cost, std)
    np.testing.assert_array_equal(np.asarray(d[M:], np.float64), cost[1:])


def test_a_basis_with_two_equal_columns_is_singular_on_the_host_too():
    A, lo, up, cost = bc.shape_model(15, 16)
    A2, vstat = bc.singular_basis(A, lo, up)
    assert int(np.sum(vstat == bc.BASIC)) == 15
    assert bc.well_conditioned(A2, lo, up, cost, vstat) is None


def test_own_model_restates_the_presolve():
    A, lo, up, cost = bc.folded_model()
    A2, lo2, up2, first, own = bc.own_model(A, lo, up, 0, 0)
    M, N = A.shape
    assert A2.shape[0] < M and A2.shape[1] == N
    assert np.sum(own < 0) == M - A2.shape[0]
    for i in np.nonzero(own[:M] < 0)[0]:
        assert np.count_nonzero(A[i]) == 1
    kept = own[:M][own[:M] >= 0]
    assert np.array_equal(kept, np.arange(len(kept)))
    assert np.all(lo2[len(kept):] >= lo[M:]) and np.all(up2[len(kept):] <= up[M:])
