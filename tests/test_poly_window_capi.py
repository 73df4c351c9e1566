"""CPU: the library exports the calls of the windowed large-facet prune (include/bslv_hip.h: bslv_poly_set_prune_window and the
calls around it, bslv_selftest_pair_blocks), the header declares them, and the Python mirror exists."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_poly_set_prune_window", "bslv_poly_get_prune_window", "bslv_poly_prune_window_stats", "bslv_selftest_pair_blocks"]


def test_window_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_window_symbols_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    # the comment in front of the calls names the environment switch, the default and what ignores the window
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_poly_set_prune_window(")], flags=re.S)[-1]
    for word in ("bslv_poly_set_prune_window", "bslv_poly_prune_window_stats", "BSLV_K2_WINDOW", "0x7FFFFFF0", "BSLV_E_ARG", "BSLV_E_CAPACITY"):
        assert word in comment, word


def test_python_mirror_has_the_calls():
    from bensolve_amd.poly import PolyEngine
    for name in ("set_prune_window", "get_prune_window", "prune_window_stats", "selftest_pair_blocks"):
        assert callable(getattr(PolyEngine, name)), name
