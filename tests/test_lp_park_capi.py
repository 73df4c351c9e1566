"""CPU: the library exports the calls of the parked tableau passes (include/bslv_hip.h: bslv_lpq_park and the calls around it,
bslv_benson_set_park), the header declares them, and the Python mirrors exist."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_park", "bslv_lpq_drop_parked", "bslv_lpq_park_stats", "bslv_lpq_set_park", "bslv_lpq_get_park",
       "bslv_benson_set_park", "bslv_benson_park_stats"]


def test_park_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_park_symbols_declared():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    # the comment in front of the lazy calls says when a parked pass is made
    comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  bslv_lpq_park(")], flags=re.S)[-1]
    for word in ("bslv_lpq_park", "bslv_lpq_drop_parked", "bslv_lpq_reset_slot", "BSLV_LP_PARK"):
        assert word in comment, word


def test_python_mirror_has_the_calls():
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    for name in ("park", "drop_parked", "set_park", "park_stats"):
        assert callable(getattr(LpEngine, name)), name
    assert callable(BensonEngine.set_park) and callable(BensonEngine.park_stats)
