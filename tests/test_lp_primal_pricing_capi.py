"""CPU: the library exports the switch between the pricing rules of the LP engine's primal steps (include/bslv_hip.h,
bslv_lpq_set_primal_pricing), its counters and the read-out of the primal Devex reference norms; the header declares them and the
environment switch; the Python mirror has the calls (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_primal_pricing", "bslv_lpq_get_primal_pricing", "bslv_lpq_last_primal_pricing_stats",
       "bslv_lpq_last_primal_pricing_norms"]
E_ARG = 2


def test_primal_pricing_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_primal_pricing_symbols_and_switch_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    assert "BSLV_LP_PRIMAL_PRICING=dantzig|devex" in txt          # the environment switch is documented beside the call


def test_python_mirror_has_the_primal_pricing_calls():
    from bensolve_amd.lp import LpEngine
    for name in ("set_primal_pricing", "get_primal_pricing", "last_primal_pricing_stats", "last_primal_pricing_norms"):
        assert callable(getattr(LpEngine, name)), name


def test_null_engine_is_refused_or_answers_the_default():
    from bensolve_amd import load_library
    lib = load_library()
    vp = ctypes.c_void_p
    lib.bslv_lpq_set_primal_pricing.argtypes = [vp, ctypes.c_int]
    lib.bslv_lpq_get_primal_pricing.argtypes = [vp]
    lib.bslv_lpq_last_primal_pricing_stats.argtypes = [vp, vp]
    lib.bslv_lpq_last_primal_pricing_norms.argtypes = [vp, ctypes.c_int, vp]
    out = (ctypes.c_long * 3)()
    t = (ctypes.c_double * 8)()
    assert lib.bslv_lpq_set_primal_pricing(None, 1) == E_ARG
    assert lib.bslv_lpq_get_primal_pricing(None) == 0
    assert lib.bslv_lpq_last_primal_pricing_stats(None, out) == E_ARG
    assert lib.bslv_lpq_last_primal_pricing_norms(None, 0, t) == E_ARG
