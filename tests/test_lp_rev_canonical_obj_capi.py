"""CPU: the library exports the per-call entry point for canonical optimal points of objective batches (include/bslv_hip.h,
bslv_lpq_solve_batch_obj_canonical), the header declares it with its twelve arguments and says what it is in the revised form, the
Python mirror exists, the dual variant's flag bit has its value, and without an engine the call answers BSLV_E_ARG (no compute)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "bslv_lpq_solve_batch_obj_canonical"


def _header():
    return open(os.path.join(ROOT, "include", "bslv_hip.h")).read()


def test_the_symbol_is_exported():
    from bensolve_amd import load_library
    assert hasattr(load_library(), NEW)


def test_the_prototype_is_in_the_header():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NEW, code)
    assert m, NEW
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 12 and args[0].startswith("bslv_lpq") and args[1].startswith("const double") and args[2] == "int B", args
    assert args[7] == "int cost_first" and args[8] == "int cost_cnt" and args[9].startswith("const double"), args
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  " + NEW)], flags=re.S)[-1]
    for word in ("REVISED", "k_select_tie_obj_rev", "neither read nor changed", "BSLV_E_ARG", "its own range"):
        assert word in comment, word


def test_the_flag_of_the_dual_variant():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bBSLV_VLP_CANONICAL_CALL\s*=\s*8\b", code)
    assert re.search(r"\bBSLV_VLP_CANONICAL\s*=\s*4\b", code)          # (stays what it is)
    from bensolve_amd import vlp
    assert '"call"' in inspect.getsource(vlp.solve_primal)


def test_python_mirror_has_the_call():
    from bensolve_amd.lp import LpEngine
    assert callable(LpEngine.solve_batch_obj_canonical)
    assert list(inspect.signature(LpEngine.solve_batch_obj_canonical).parameters)[:6] == ["self", "ddir", "src", "dst", "cost_first", "costs"]


def test_no_engine_is_a_bad_argument():
    from bensolve_amd import load_library
    lib = load_library()
    fn = getattr(lib, NEW)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    fn.restype = ctypes.c_int
    assert fn(None, None, 0, None, None, None, None, 0, 1, None, None, None) == 2          # BSLV_E_ARG
    assert NEW in lib.bslv_last_error().decode()
