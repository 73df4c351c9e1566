"""CPU: the consistency check of the polyhedron engine at the ABI -- the header declares bslv_poly_check and bslv_poly_debug_corrupt
with the signature the callers use, the library exports them, poly__polyck is still exported, and the calls that need no device
(null engine, bad arguments) are refused."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_poly_check", "bslv_poly_debug_corrupt"]


def _header():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_check_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW + ["poly__polyck"] if not hasattr(lib, s)]
    assert not missing, missing


def test_check_symbols_declared():
    txt, code = _header()
    flat = re.sub(r"\s+", " ", code)
    assert "int bslv_poly_check(bslv_poly *h, double tol , int row_first, int row_count , long out[12], double worst[2] , int *offenders , int max_off, int *n_off);" in flat
    assert "int bslv_poly_debug_corrupt(bslv_poly *h, int what, int a, int b, double x);" in flat
    # the comment in front of the call says what the twelve fields are, that the call only reads, and that nothing out of range is followed
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_poly_check(")], flags=re.S)[-1]
    for word in ["out[%d]" % k for k in range(12)] + ["Read-only", "never dereferences", "POLY_EPS", "BSLV_E_ARG", "BSLV_E_STATE", "row_first", "worst[1]"]:
        assert word in comment, word


def test_refused_without_a_device():
    from bensolve_amd import load_library
    lib = load_library()
    lib.bslv_poly_check.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.bslv_poly_debug_corrupt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    out = (ctypes.c_long * 12)()
    assert lib.bslv_poly_check(None, 0.0, 0, -1, out, None, None, 0, None) == 2          # BSLV_E_ARG
    assert b"bslv_poly_check" in lib.bslv_last_error()
    assert lib.bslv_poly_debug_corrupt(None, 0, 0, 0, 0.0) == 2


def test_python_mirror_and_callers():
    from bensolve_amd.poly import PolyEngine
    for name in ("check", "debug_corrupt"):
        assert callable(getattr(PolyEngine, name)), name
    assert len(PolyEngine.CHECK_FIELDS) == 12
    # the command-line driver audits under -t, the Benson driver under BSLV_POLY_CHECK, the compat layer in poly__polyck
    src = lambda *p: open(os.path.join(ROOT, "bensolve_amd", "csrc", *p)).read()
    assert "bslv_poly_check(" in src("host", "bensolve_hip_main.c") and "polyhedron check:" in src("host", "bensolve_hip_main.c")
    assert "bslv_poly_check(" in src("benson_driver.hip") and "BSLV_POLY_CHECK" in src("benson_driver.hip")
    assert "bslv_poly_check(" in src("poly_compat.hip")
