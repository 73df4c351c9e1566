"""CPU: the device-side LP certificate at the ABI -- the header declares bslv_lpq_certify, its statistics, the test hook and the Benson
driver's switch with the signatures the callers use and names the five kinds and the six default tolerances, the library exports
them, the Python mirrors exist, and the calls that need no device (a null engine) are refused."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_certify", "bslv_lpq_last_certify_stats", "bslv_lpq_debug_poke", "bslv_benson_set_certify", "bslv_benson_get_certify",
       "bslv_benson_certify_stats"]


def _header():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_certify_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_certify_symbols_declared():
    txt, code = _header()
    flat = re.sub(r"\s+", " ", code)
    assert ("int bslv_lpq_certify(bslv_lpq *h, int B, const int *slot, const double *vlo, const double *vup, int cost_first, int cost_cnt, "
            "const double *costs, const double *tol, double *res, int *at, int *verdict);") in flat
    assert "int bslv_lpq_last_certify_stats(const bslv_lpq *h, long out[3]);" in flat
    assert "int bslv_lpq_debug_poke(bslv_lpq *h, int slot, int what, int var, double delta);" in flat
    assert "int bslv_benson_set_certify(bslv_benson *h, int on);" in flat
    assert "int bslv_benson_get_certify(const bslv_benson *h);" in flat
    assert "int bslv_benson_certify_stats(const bslv_benson *h, long counts[3], double worst[5]);" in flat
    # the comment in front of the call names the five kinds, the six defaults, that the call only reads, and its errors
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int bslv_lpq_certify(")], flags=re.S)[-1]
    for word in ["rows", "feas", "dj", "side", "gap", "Read-only", "1e-9, 1e-8, 1e-8, 1e-7", "tol[4] = 1e-9", "tol[5] = 1e-9", "(1 + |z|)", "BSLV_E_ARG",
                 "bslv_lpq_get_obj", "model AS GIVEN", "BSLV_LP_CERTIFY_TIMING", "verdict[b]", "at[b*5 + k]"]:
        assert word in comment, word
    assert "BSLV_LP_CERTIFY=1" in txt


def test_refused_without_a_device():
    from bensolve_amd import load_library
    lib = load_library()
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.bslv_lpq_certify.argtypes = [vp, i, vp, vp, vp, i, i, vp, vp, vp, vp, vp]
    lib.bslv_lpq_debug_poke.argtypes = [vp, i, i, i, d]
    lib.bslv_benson_set_certify.argtypes = [vp, i]
    lib.bslv_benson_get_certify.argtypes = [vp]
    lib.bslv_benson_certify_stats.argtypes = [vp, vp, vp]
    lib.bslv_lpq_last_certify_stats.argtypes = [vp, vp]
    res = (ctypes.c_double * 5)()
    slot = (ctypes.c_int * 1)(0)
    assert lib.bslv_lpq_certify(None, 1, slot, None, None, 0, 0, None, None, res, None, None) == 2          # BSLV_E_ARG
    assert b"bslv_lpq_certify" in lib.bslv_last_error()
    assert lib.bslv_lpq_debug_poke(None, 0, 0, 0, 1e-6) == 2
    assert b"bslv_lpq_debug_poke" in lib.bslv_last_error()
    assert lib.bslv_benson_set_certify(None, 1) == 2
    assert b"bslv_benson_set_certify" in lib.bslv_last_error()
    assert lib.bslv_benson_get_certify(None) == 0
    assert lib.bslv_benson_certify_stats(None, None, None) == 2
    assert lib.bslv_lpq_last_certify_stats(None, None) == 2


def test_python_mirror_and_callers():
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    for name in ("certify", "last_certify_stats", "debug_poke"):
        assert callable(getattr(LpEngine, name)), name
    for name in ("set_certify", "get_certify", "certify_stats"):
        assert callable(getattr(BensonEngine, name)), name
    src = lambda *p: open(os.path.join(ROOT, "bensolve_amd", "csrc", *p)).read()
    # the kernels live in their own file, the Benson driver certifies under its switch, the group and tile sizes are named constants
    assert '#include "lp_certify.inc"' in src("lp_engine.hip")
    assert "bslv_lpq_certify(" in src("benson_driver.hip") and "BSLV_LP_CERTIFY" in src("benson_driver.hip")
    inc = src("lp_certify.inc")
    for word in ("constexpr int CERT_G", "constexpr int CERT_TO", "constexpr int CERT_TK", "constexpr int CERT_SR", "fma(", "-ffp-contract=off", "BSLV_LP_CERTIFY_TIMING"):
        assert word in inc, word
    assert "atomicAdd" not in inc          # (fixed summation order: no atomics in the arithmetic)
