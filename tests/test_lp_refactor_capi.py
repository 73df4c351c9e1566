"""CPU: the library exports the refactorisation of the revised LP form (include/bslv_hip.h: bslv_lpq_refactor, the in-call rescue
switch bslv_lpq_set_refactor and the test support around them), the header declares them and LpEngine mirrors them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_refactor", "bslv_lpq_set_refactor", "bslv_lpq_get_refactor", "bslv_lpq_last_refactor_stats",
       "bslv_lpq_get_inverse", "bslv_lpq_debug_perturb_inverse", "bslv_lpq_debug_swap_heads"]


def test_refactor_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_refactor_symbols_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    # the comment in front of the entry point says what happens to slots of objective batches, and names the environment switches
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_lpq_refactor")], flags=re.S)[-1]
    assert "own-cost" in comment and "BSLV_LP_REFACTOR" in comment and "tableau form" in comment
    assert "BSLV_LP_REV_DRIFT" in txt


def test_python_mirror_has_the_methods():
    from bensolve_amd.lp import LpEngine
    for name in ("refactor", "set_refactor", "get_refactor", "last_refactor_stats", "get_inverse", "debug_perturb_inverse", "debug_swap_heads"):
        assert callable(getattr(LpEngine, name)), name


def test_entry_points_refuse_a_missing_engine():
    """no device needed: every new entry point checks its handle first"""
    import ctypes
    from bensolve_amd import load_library
    lib = load_library()
    lib.bslv_lpq_refactor.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.bslv_lpq_set_refactor.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.bslv_lpq_get_refactor.argtypes = [ctypes.c_void_p]
    lib.bslv_lpq_get_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.bslv_lpq_debug_perturb_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    lib.bslv_lpq_last_refactor_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.bslv_lpq_debug_swap_heads.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert lib.bslv_lpq_refactor(None, 0, None, None) == 2          # BSLV_E_ARG
    assert lib.bslv_lpq_set_refactor(None, 1) == 2
    assert lib.bslv_lpq_get_refactor(None) == 0
    assert lib.bslv_lpq_get_inverse(None, 0, None, None) == 2
    assert lib.bslv_lpq_debug_perturb_inverse(None, 0, 1e-6) == 2
    assert lib.bslv_lpq_last_refactor_stats(None, None) == 2
    assert lib.bslv_lpq_debug_swap_heads(None, 0, 0, 0) == 2
