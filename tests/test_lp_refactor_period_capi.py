"""CPU: the library exports the periodic refactorisation of the revised LP form and the age of a slot's matrix (include/bslv_hip.h:
bslv_lpq_set_refactor_period, bslv_lpq_get_refactor_period, bslv_lpq_slot_age, bslv_lpq_last_period_stats), the header declares them
and LpEngine mirrors them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_refactor_period", "bslv_lpq_get_refactor_period", "bslv_lpq_slot_age", "bslv_lpq_last_period_stats"]


def test_period_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_period_symbols_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    # the comment in front of the entry points names the environment variable, the tableau form's answer and the bound on the age
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_lpq_set_refactor_period")], flags=re.S)[-1]
    assert "BSLV_LP_REFACTOR_EVERY" in comment and "tableau form" in comment and "2 K + KP" in comment


def test_python_mirror_has_the_methods():
    from bensolve_amd.lp import LpEngine
    for name in ("set_refactor_period", "get_refactor_period", "slot_age", "last_period_stats"):
        assert callable(getattr(LpEngine, name)), name


def test_entry_points_refuse_a_missing_engine():
    """no device needed: every new entry point checks its handle first"""
    import ctypes
    from bensolve_amd import load_library
    lib = load_library()
    lib.bslv_lpq_set_refactor_period.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.bslv_lpq_get_refactor_period.argtypes = [ctypes.c_void_p]
    lib.bslv_lpq_slot_age.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.bslv_lpq_last_period_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    age = ctypes.c_long(7)
    out = (ctypes.c_long * 4)()
    assert lib.bslv_lpq_set_refactor_period(None, 5) == 2          # BSLV_E_ARG
    assert lib.bslv_lpq_set_refactor_period(None, 0) == 2
    assert lib.bslv_lpq_get_refactor_period(None) == 0
    assert lib.bslv_lpq_slot_age(None, 0, ctypes.byref(age)) == 2
    assert lib.bslv_lpq_last_period_stats(None, out) == 2
