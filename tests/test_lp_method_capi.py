"""CPU: the library exports the switch between the simplex methods of the LP engine (include/bslv_hip.h, bslv_lpq_set_method)
and the counters of its primal phase 1, and the header declares them (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_method", "bslv_lpq_get_method", "bslv_lpq_last_phase1_stats"]


def test_method_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_method_symbols_and_constants_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    m = re.search(r"enum\s*\{([^}]*BSLV_LP_METHOD_DUAL[^}]*)\}", code)
    assert m, "enum of the methods"
    vals = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert vals == {"BSLV_LP_METHOD_DUAL": 0, "BSLV_LP_METHOD_PRIMAL": 1, "BSLV_LP_METHOD_REPAIR": 2}


def test_python_mirror_has_the_method():
    from bensolve_amd.lp import LpEngine
    assert callable(LpEngine.set_method) and callable(LpEngine.get_method)
