"""CPU: the library exports the per-call simplex method of the LP engine (include/bslv_hip.h, bslv_lpq_solve_batch_method: the way
to PRIMAL and REPAIR in the revised form), the header declares it and the Python mirror has it (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "bslv_lpq_solve_batch_method"


def test_solve_batch_method_exported():
    from bensolve_amd import load_library
    lib = load_library()
    assert hasattr(lib, NEW)


def test_solve_batch_method_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NEW, code)
    assert m, NEW
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and re.search(r"\bint\s+method$", args[1]), args      # (h, method, B, src, dst, vlo, vup, status, iters)


def test_python_mirror_has_solve_batch_method():
    from bensolve_amd.lp import LpEngine
    assert callable(LpEngine.solve_batch_method)
