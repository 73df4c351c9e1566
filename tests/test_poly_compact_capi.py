"""CPU: the library exports the compaction calls (include/bslv_hip.h: bslv_poly_garbage, bslv_poly_compact,
bslv_poly_last_compact_stats, bslv_benson_set_compact, bslv_benson_compact_stats), the header declares them and states their rules in
the comments in front of them, and the Python mirror exists."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_poly_garbage", "bslv_poly_compact", "bslv_poly_last_compact_stats", "bslv_benson_set_compact", "bslv_benson_compact_stats"]


def test_compact_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def _comment_before(txt, decl):
    return re.findall(r"/\*(.*?)\*/", txt[:txt.index(decl)], flags=re.S)[-1]


def test_compact_symbols_declared_and_their_rules_stated():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    poly = _comment_before(txt, "int  bslv_poly_garbage(")
    for word in ("bslv_poly_garbage", "bslv_poly_compact", "bslv_poly_last_compact_stats", "BSLV_POLY_COMPACT", "new_of_old", "BSLV_E_STATE",
                 "BSLV_E_NODEVICE", "BSLV_E_ARG", "MONOTONE", "STALE IDS", "old + new", "DROPPED"):
        assert word in poly, word
    drv = _comment_before(txt, "int  bslv_benson_set_compact(")
    for word in ("BSLV_POLY_COMPACT", "new_of_old", "65536", "BSLV_E_ARG", "PIPELINED MODE", "not applied yet", "SEVERAL RANKS", "STALE IDS",
                 "bslv_benson_compact_stats"):
        assert word in drv, word


def test_python_mirror_has_the_calls():
    from bensolve_amd.poly import PolyEngine
    from bensolve_amd.benson import BensonEngine
    for name in ("garbage", "compact", "last_compact_stats"):
        assert callable(getattr(PolyEngine, name)), name
    for name in ("set_compact", "compact_stats"):
        assert callable(getattr(BensonEngine, name)), name
