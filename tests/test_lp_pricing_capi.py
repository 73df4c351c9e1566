"""CPU: the library exports the switch between the pricing rules of the LP engine's dual steps (include/bslv_hip.h,
bslv_lpq_set_pricing), its counters and the read-out of the Devex reference norms; the header declares them (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_pricing", "bslv_lpq_get_pricing", "bslv_lpq_last_pricing_stats", "bslv_lpq_last_pricing_norms"]
E_ARG = 2


def test_pricing_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_pricing_symbols_and_constants_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    m = re.search(r"enum\s*\{([^}]*BSLV_LP_PRICING_DANTZIG[^}]*)\}", code)
    assert m, "enum of the pricing rules"
    vals = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert vals == {"BSLV_LP_PRICING_DANTZIG": 0, "BSLV_LP_PRICING_DEVEX": 1}
    assert "BSLV_LP_PRICING=dantzig|devex" in txt          # the environment switch is documented beside the call


def test_python_mirror_has_the_pricing_calls():
    from bensolve_amd.lp import LpEngine
    for name in ("set_pricing", "get_pricing", "last_pricing_stats", "last_pricing_norms"):
        assert callable(getattr(LpEngine, name)), name


def test_null_engine_is_refused_or_answers_the_default():
    from bensolve_amd import load_library
    lib = load_library()
    vp = ctypes.c_void_p
    lib.bslv_lpq_set_pricing.argtypes = [vp, ctypes.c_int]
    lib.bslv_lpq_get_pricing.argtypes = [vp]
    lib.bslv_lpq_last_pricing_stats.argtypes = [vp, vp]
    lib.bslv_lpq_last_pricing_norms.argtypes = [vp, ctypes.c_int, vp]
    out = (ctypes.c_long * 3)()
    s = (ctypes.c_double * 4)()
    assert lib.bslv_lpq_set_pricing(None, 1) == E_ARG
    assert lib.bslv_lpq_get_pricing(None) == 0
    assert lib.bslv_lpq_last_pricing_stats(None, out) == E_ARG
    assert lib.bslv_lpq_last_pricing_norms(None, 0, s) == E_ARG
