"""The Benson driver parks the tableau passes of the slots it keeps (bslv_benson_set_park, default on) instead of making them at the
end of apply().  Nothing the algorithm sees may change: a small covering problem run to termination with a pool so small that
parents are evicted all the time gives the same vertex and facet sets (SHA-256 over the canonical dump), the same totals of LPs,
pivots and cuts and the same warm-start statistics with the switch on and off -- while the engine's own statistics show that passes
were dropped with their evicted slots and that parked children were given their tableau because their parent was about to be
overwritten."""
import functools
import hashlib
import os

import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine
import poly_harness as ph

pytestmark = pytest.mark.gpu
BATCH, POOL = 16, 48      # 30 x 15, q = 3: far more cuts than slots; take_slot evicts six parents at a time


def _digest(eng, decimals=6):
    eng.poly_call("dual_adjacency")
    can = ph.canonical(eng.poly_dump(), decimals=decimals)
    h = hashlib.sha256()
    for k in sorted(can):
        v = can[k]
        if isinstance(v, np.ndarray):
            a = np.round(v, decimals) + 0.0 if v.dtype.kind == "f" else v
            h.update(k.encode()); h.update(np.ascontiguousarray(a).tobytes())
        else:
            h.update(k.encode()); h.update(np.array(sorted(v), np.int64).tobytes())
    return h.hexdigest(), len(can["X"]), len(can["Y"])


@functools.lru_cache(maxsize=None)
def _run(park, retry=False):
    prob = synth.covering_vlp(30, 15, 3, 5)
    old = os.environ.get("BSLV_FORCE_RETRY")
    if retry:
        os.environ["BSLV_FORCE_RETRY"] = "1"          # (read at every batch: every other LP goes through the driver's retry)
    try:
        eng = BensonEngine(prob, eps=1e-7, pool_slots=POOL)
        try:
            eng.set_park(park)
            assert eng.start() == 0
            steps = eng.run(BATCH)
            return dict(steps=steps, totals=eng.totals(), starts=eng.start_stats(), park=eng.park_stats(), sets=_digest(eng))
        finally:
            eng.close()
    finally:
        if retry:
            if old is None:
                del os.environ["BSLV_FORCE_RETRY"]
            else:
                os.environ["BSLV_FORCE_RETRY"] = old


def test_a_run_with_evictions_ends_the_same_with_park_on_and_off():
    on, off = _run(1), _run(0)
    print("park on:", on)
    print("park off:", off)
    assert off["park"] == dict(parked=0, for_child=0, forced=0, dropped=0, live=0)
    ps = on["park"]
    assert ps["parked"] > 0 and ps["dropped"] > 0 and ps["forced"] >= 1, ps
    assert ps["parked"] == ps["for_child"] + ps["forced"] + ps["dropped"] + ps["live"], ps
    assert on["starts"]["root"] + on["starts"]["nearest"] > 0, on["starts"]      # (children of evicted parents: evictions did happen)
    for k in ("sets", "totals", "starts", "steps"):
        assert on[k] == off[k], (k, on[k], off[k])


def test_the_retry_of_the_driver_meets_parked_slots():
    """BSLV_FORCE_RETRY=1: a second solve_batch arrives while the slots of the first are still open, then apply() parks"""
    on, off = _run(1, True), _run(0, True)
    print("park on:", on)
    assert on["park"]["parked"] > 0
    for k in ("sets", "totals", "starts", "steps"):
        assert on[k] == off[k], (k, on[k], off[k])
