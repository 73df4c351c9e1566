"""CPU: the library exports the per-call entry point for canonical optimal duals (include/bslv_hip.h, bslv_lpq_solve_batch_canonical),
the header declares it with its nine arguments and says what it is in the revised form, the Python mirror exists, and without an engine
the call answers BSLV_E_ARG (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "bslv_lpq_solve_batch_canonical"


def test_the_symbol_is_exported():
    from bensolve_amd import load_library
    assert hasattr(load_library(), NEW)


def test_the_prototype_is_in_the_header():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NEW, code)
    assert m, NEW
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[0].startswith("bslv_lpq") and args[1].startswith("const double") and args[2] == "int B", args
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  " + NEW)], flags=re.S)[-1]
    for word in ("REVISED", "k_select_tie_rev", "neither read nor changed", "BSLV_E_ARG"):
        assert word in comment, word
    # the engine-wide switches keep their refusal in the revised form
    assert "the revised form answers BSLV_E_ARG" in txt


def test_python_mirror_has_the_call():
    from bensolve_amd.lp import LpEngine
    assert callable(LpEngine.solve_batch_canonical)


def test_no_engine_is_a_bad_argument():
    from bensolve_amd import load_library
    lib = load_library()
    fn = getattr(lib, NEW)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6
    fn.restype = ctypes.c_int
    assert fn(None, None, 0, None, None, None, None, None, None) == 2          # BSLV_E_ARG
    assert NEW in lib.bslv_last_error().decode()
