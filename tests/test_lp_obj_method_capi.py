"""CPU: the library exports the simplex method of objective batches per call (include/bslv_hip.h, bslv_lpq_solve_batch_obj_method and
its counters) and the method switch of the Benson driver (bslv_benson_set_lp_method), the header declares them with the documented
signatures beside the method enum, and the Python mirrors have them (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("bslv_lpq_solve_batch_obj_method", "bslv_lpq_last_obj_method_stats")
DRIVER = ("bslv_benson_set_lp_method", "bslv_benson_get_lp_method", "bslv_benson_lp_method_stats")
VLP = ("bslv_vlp_last_lp_method_stats", "bslv_lp_compat_method")


def _code():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _code())
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    for name in ENGINE + DRIVER + VLP:
        assert hasattr(lib, name), name


def test_solve_batch_obj_method_declared():
    # (h, method, B, src, dst, vlo, vup, cost_first, cost_cnt, costs, status, iters): solve_batch_obj's arguments behind the method
    args = _args("bslv_lpq_solve_batch_obj_method")
    assert len(args) == 12, args
    assert args[0] == "bslv_lpq *h" and args[1] == "int method" and args[2] == "int B", args
    assert args[7] == "int cost_first" and args[8] == "int cost_cnt" and args[9] == "const double *costs", args
    assert args[10] == "int *status" and args[11] == "int *iters", args
    assert _args("bslv_lpq_solve_batch_obj")[1:] == args[2:], "solve_batch_obj's own arguments"
    assert _args("bslv_lpq_last_obj_method_stats") == ["const bslv_lpq *h", "long out[4]"]


def test_driver_switch_declared():
    assert _args("bslv_benson_set_lp_method") == ["bslv_benson *h", "int method"]
    assert _args("bslv_benson_get_lp_method") == ["const bslv_benson *h"]
    assert _args("bslv_benson_lp_method_stats") == ["const bslv_benson *h", "long out[3]"]


def test_method_enum_in_the_header():
    code = _code()
    m = re.search(r"enum\s*\{\s*BSLV_LP_METHOD_DUAL\s*=\s*0\s*,\s*BSLV_LP_METHOD_PRIMAL\s*=\s*1\s*,\s*BSLV_LP_METHOD_REPAIR\s*=\s*2\s*\}", code)
    assert m, "the method enum"


def test_bad_arguments_change_nothing():
    """h == NULL and a method outside 0 .. 2 are BSLV_E_ARG before anything is looked at (no engine, no GPU)"""
    import ctypes
    from bensolve_amd import load_library
    lib = load_library()
    E_ARG = -1
    f = lib.bslv_lpq_solve_batch_obj_method
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    f.restype = ctypes.c_int
    rc = f(None, 0, 0, None, None, None, None, 0, 1, None, None, None)
    assert rc != 0
    lib.bslv_lpq_last_obj_method_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.bslv_lpq_last_obj_method_stats(None, None) == rc
    lib.bslv_benson_set_lp_method.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.bslv_benson_set_lp_method(None, 0) == rc
    lib.bslv_benson_get_lp_method.argtypes = [ctypes.c_void_p]
    assert lib.bslv_benson_get_lp_method(None) == E_ARG          # (-1 is also "unset": what a missing engine has)


def test_python_mirrors():
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    assert callable(LpEngine.solve_batch_obj_method) and callable(LpEngine.last_obj_method_stats)
    assert callable(BensonEngine.set_lp_method) and callable(BensonEngine.get_lp_method) and callable(BensonEngine.lp_method_stats)


def test_vlp_flag_helpers_and_stats_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+BSLV_VLP_LP_METHOD\(phase,\s*m\)\s+\(\(\(m\)\s*\+\s*1\)\s*<<\s*\(4\s*\+\s*2\s*\*\s*\(phase\)\)\)", code), "BSLV_VLP_LP_METHOD"
    assert "BSLV_VLP_LP_METHOD_OF(flags, phase)" in code
    assert _args("bslv_vlp_last_lp_method_stats") == ["long out[5][3]"]
    # two bits per phase above the four existing flags, 0 = not given: the Python mirror builds the same bits
    from bensolve_amd.vlp import lp_method_flags
    assert lp_method_flags(None) == 0 and lp_method_flags(("auto", None, "auto")) == 0
    assert lp_method_flags(("dual", None, None)) == 1 << 4 and lp_method_flags((None, "primal", None)) == 2 << 6 and lp_method_flags((None, None, "repair")) == 3 << 8
    assert lp_method_flags(("primal", "dual", "repair")) & 15 == 0


def test_compat_mapping_is_the_references():
    """lp_set_options' table (bslv_lp.c:153-217) through bslv_lp_compat_method: the option of the phase, or the phase's own method"""
    import ctypes
    from bensolve_amd import load_library
    lib = load_library()

    class Opt(ctypes.Structure):
        _fields_ = [("p0", ctypes.c_int), ("p1", ctypes.c_int), ("p2", ctypes.c_int), ("msg", ctypes.c_int)]
    f = lib.bslv_lp_compat_method
    f.argtypes = [ctypes.POINTER(Opt), ctypes.c_int, ctypes.c_int]
    PRIMAL_SIMPLEX, DUAL_SIMPLEX, DUAL_PRIMAL_SIMPLEX, AUTO = range(4)
    DUAL, PRIMAL, REPAIR = 0, 1, 2
    auto = Opt(AUTO, AUTO, AUTO, 0)
    assert [f(auto, ph, REPAIR) for ph in range(5)] == [REPAIR, DUAL, PRIMAL, DUAL, PRIMAL]
    o = Opt(PRIMAL_SIMPLEX, DUAL_PRIMAL_SIMPLEX, DUAL_SIMPLEX, 0)
    assert [f(o, ph, DUAL) for ph in range(5)] == [PRIMAL, REPAIR, REPAIR, DUAL, DUAL]
    assert f(auto, 5, 0) == -1 and f(Opt(7, AUTO, AUTO, 0), 0, 0) == -1
