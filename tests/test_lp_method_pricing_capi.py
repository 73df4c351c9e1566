"""CPU: the library exports the pricing rules per call (include/bslv_hip.h, bslv_lpq_solve_batch_method_priced) and the Benson driver's
switch for them (bslv_benson_set_lp_pricing, BSLV_BENSON_LP_PRICING), the header declares them with the documented signatures, the
Python mirrors have them, and a missing engine or a rule out of range is BSLV_E_ARG (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("bslv_lpq_solve_batch_method_priced",)
DRIVER = ("bslv_benson_set_lp_pricing", "bslv_benson_get_lp_pricing")
E_ARG = 2


def _text():
    return open(os.path.join(ROOT, "include", "bslv_hip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _text(), flags=re.S)


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _code())
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    for name in ENGINE + DRIVER:
        assert hasattr(lib, name), name


def test_declared_in_the_header():
    # (h, method, dual_rule, primal_rule, B, src, dst, vlo, vup, status, iters): solve_batch_method's arguments with the two rules behind the method
    args = _args("bslv_lpq_solve_batch_method_priced")
    assert args[:4] == ["bslv_lpq *h", "int method", "int dual_rule", "int primal_rule"], args
    assert args[4:] == _args("bslv_lpq_solve_batch_method")[2:], args
    assert _args("bslv_benson_set_lp_pricing") == ["bslv_benson *h", "int dual_rule", "int primal_rule"]
    assert _args("bslv_benson_get_lp_pricing") == ["const bslv_benson *h", "int *dual_rule", "int *primal_rule"]
    txt = _text()
    assert "BSLV_BENSON_LP_PRICING" in txt
    # the two paragraphs that said no Devex instance carries the revised form's phase 1 now name the call
    assert "no Devex instance carries" not in txt
    flat = re.sub(r"\s*\n\s*\*\s*", " ", txt)          # (comment lines joined)
    assert flat.count("only through bslv_lpq_solve_batch_method_priced") >= 2


def test_python_mirrors():
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    assert callable(LpEngine.solve_batch_method_priced)
    assert callable(BensonEngine.set_lp_pricing) and callable(BensonEngine.get_lp_pricing)


def test_null_handles_and_bad_rules_are_refused():
    """h == NULL is BSLV_E_ARG before anything is looked at (no engine, no GPU); so is, with h == NULL, every rule -- the range of the
    rules on a live engine is the GPU suite's (tests/test_lp_rev_p1_pricing_gpu.py, tests/test_benson_lp_pricing_gpu.py)"""
    from bensolve_amd import load_library
    lib = load_library()
    f = lib.bslv_lpq_solve_batch_method_priced
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
    f.restype = ctypes.c_int
    st = (ctypes.c_int * 1)(-7)
    for method, dr, pr in ((1, 0, 1), (1, 2, 0), (1, 0, -1), (3, 0, 0), (-1, 1, 1)):
        assert f(None, method, dr, pr, 1, None, None, None, None, st, None) == E_ARG, (method, dr, pr)
    assert st[0] == -7
    lib.bslv_benson_set_lp_pricing.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    for dr, pr in ((0, 1), (-1, -1), (2, 0), (0, -1)):
        assert lib.bslv_benson_set_lp_pricing(None, dr, pr) == E_ARG
    lib.bslv_benson_get_lp_pricing.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    d, p = ctypes.c_int(5), ctypes.c_int(5)
    assert lib.bslv_benson_get_lp_pricing(None, ctypes.byref(d), ctypes.byref(p)) == E_ARG and (d.value, p.value) == (5, 5)
