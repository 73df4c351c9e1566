"""CPU: the library exports the switch for canonical optimal duals (include/bslv_hip.h, bslv_lpq_set_canonical and
bslv_benson_set_canonical), the header declares it and cites where the reference takes the duals from, the Python mirrors exist, and
without a device the constructors still answer BSLV_E_NODEVICE (no compute)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bslv_lpq_set_canonical", "bslv_lpq_get_canonical", "bslv_lpq_last_canonical_stats",
       "bslv_benson_set_canonical", "bslv_benson_get_canonical", "bslv_benson_canonical_stats"]


def test_canonical_symbols_exported():
    from bensolve_amd import load_library
    lib = load_library()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_canonical_symbols_declared_with_their_source():
    txt = open(os.path.join(ROOT, "include", "bslv_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), s
    # the doc comments in front of the two switches name the line the cut's w comes from
    for s in ("bslv_lpq_set_canonical", "bslv_benson_set_canonical"):
        comment = re.findall(r"/\*(.*?)\*/", txt[:txt.index("int  " + s)], flags=re.S)[-1]
        assert "bslv_algs.c:1050" in comment, s


def test_python_mirror_has_the_switch():
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    assert callable(LpEngine.set_canonical) and callable(LpEngine.get_canonical) and callable(LpEngine.last_canonical_stats)
    assert callable(BensonEngine.set_canonical)


def test_constructors_still_fail_without_a_device():
    import numpy as np
    import torch
    from bensolve_amd import load_library
    from bensolve_amd._lib import BslvError
    from bensolve_amd.lp import LpEngine
    from bensolve_amd.benson import BensonEngine
    import canonical_cases as cc
    lib = load_library()
    if torch.cuda.is_available():
        return
    assert lib.bslv_device_count() == 0
    old = os.environ.get("BSLV_CANONICAL_DUAL")
    os.environ["BSLV_CANONICAL_DUAL"] = "1"            # (the environment switch must not get in front of the device check)
    try:
        for make in (lambda: LpEngine(1, 1, np.ones((1, 1)), np.zeros(2), np.ones(2), np.zeros(2), 0, 1, 2),
                     lambda: BensonEngine(cc.octahedron_vlp(), eps=1e-9, pool_slots=8)):
            try:
                make()
            except BslvError as e:
                assert "error 1:" in str(e) and "device" in str(e).lower(), str(e)      # BSLV_E_NODEVICE
            else:
                raise AssertionError("engine construction must fail without a GPU: there is no CPU fallback")
    finally:
        if old is None:
            del os.environ["BSLV_CANONICAL_DUAL"]
        else:
            os.environ["BSLV_CANONICAL_DUAL"] = old
