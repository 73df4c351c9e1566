"""bslv_lpq_park: the tableau pass of a slot the caller keeps is postponed until the slot is used (include/bslv_hip.h).  The pass
is the same pass on the same inputs, so every case below runs twice on one kind of engine -- park on, and park off, where
bslv_lpq_park materialises at once -- and compares every array byte for byte."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine

pytestmark = pytest.mark.gpu
B = 96


@functools.lru_cache(maxsize=None)
def _setup():
    prob = synth.covering_vlp(200, 100, 3, 1)
    model = P2Model(prob)
    rng = np.random.default_rng(4)
    n = prob["n"]                                      # (the points of test_lazy_tableaux_give_the_same_lps_and_the_same_children)
    X = rng.random((B, n)) * (3.0 / n) + 1.0 / n
    Y = X @ prob["P"].T
    V = Y * rng.uniform(0.2, 1.2, size=(B, 1)) + rng.normal(scale=0.05, size=Y.shape)
    return prob, model, V


def _engine(park):
    prob, model, V = _setup()
    eng = LpEngine.from_model(model, pool_slots=4 * B + 2)
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), model.ub_for(V[:1]))
    assert st0[0] == 4
    eng.set_lazy(1)
    eng.set_park(park)
    return eng


def _solve(eng, src, dst, V):
    """one batch; what the getters say about its slots, as a list of arrays"""
    prob, model, _ = _setup()
    src = np.asarray(src, np.int32)
    dst = np.asarray(dst, np.int32)
    st, it = eng.solve_batch(src, dst, np.full((len(src), model.r), -np.inf), model.ub_for(V))
    assert np.all(st == 4), st
    return [st.copy(), it.copy()] + _read(eng, dst)


def _read(eng, slots):
    prob, model, _ = _setup()
    return [eng.obj(slots).copy(), eng.dual(slots, model.w_first, model.q).copy(), eng.primal(slots, model.y_first, model.q).copy(),
            eng.primal(slots, model.M, prob["n"]).copy()]


def _keep(eng, slots):
    """what the Benson driver does at the end of apply()"""
    eng.park(slots)
    eng.discard_pending()


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), "array %d differs" % k


def _both(scenario):
    out = {}
    for park in (1, 0):
        eng = _engine(park)
        try:
            out[park] = scenario(eng) + (eng.park_stats(), eng.lazy_stats())
        finally:
            eng.close()
    _same(out[1][0], out[0][0])
    assert out[0][-2] == dict(parked=0, for_child=0, forced=0, dropped=0, live=0), out[0][-2]
    return out[1], out[0]


DST1 = np.arange(1, B + 1, dtype=np.int32)
KEEP = DST1[::3].copy()


def _two_generations(eng):
    _, _, V = _setup()
    res = _solve(eng, np.zeros(B, np.int32), DST1, V)
    _keep(eng, KEEP)
    res += _solve(eng, KEEP, np.arange(B + 1, B + 1 + len(KEEP)), V[::3] * 1.05 + 0.02)
    eng.discard_pending()
    return (res,)


@functools.lru_cache(maxsize=None)
def _case1():
    return _both(_two_generations)


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_children_of_parked_slots_are_the_same_lps():
    """every third slot parked, a second generation solved from them: statuses, pivots, objective, w, y and x of both generations"""
    on, off = _case1()
    ps = on[-2]
    print("park on:", ps, on[-1], "park off:", off[-1])
    assert ps["parked"] >= 1
    # one pass per distinct source that needed one -- which the engine without park counts as its passes on request (MI355X: 27 of the
    # 32 sources; the other five had passed once and ended with nothing pending, so they are not parked: they have their tableau)
    assert ps["for_child"] == ps["parked"] == off[-1]["on_request"] <= len(set(KEEP.tolist())), (ps, off[-1])
    assert on[-1]["on_request"] == off[-1]["on_request"], (on[-1], off[-1])
    assert ps["forced"] == 0 and ps["live"] == ps["parked"] - ps["for_child"] - ps["dropped"]


def test_a_batch_that_uses_no_parked_slot_makes_no_pass():
    _, _, V = _setup()
    first = _case1()[0][0][2:6]                          # what the getters said about DST1 after the first generation

    def scenario(eng):
        res = _solve(eng, np.zeros(B, np.int32), DST1, V)
        _keep(eng, KEEP)
        before = eng.lazy_stats()["on_request"], eng.park_stats()
        res += _solve(eng, np.zeros(32, np.int32), np.arange(B + 1, B + 33), V[:32] * 0.97)
        launches = eng.last_stats()["launches"], eng.last_stats()["lockstep_iters"]
        eng.discard_pending()
        after = eng.lazy_stats()["on_request"], eng.park_stats()
        got = _read(eng, DST1)
        return res + got, before, after, launches, got

    on, off = _both(scenario)
    _, before, after, launches, got = on[:5]
    assert before == after and before[1]["live"] == before[1]["parked"] >= 1, (before, after)
    assert launches[0] == launches[1], launches          # one k_flush launch per round, none for a parked slot
    _same(got, first)


def test_a_source_about_to_be_overwritten_gives_its_parked_children_their_tableau_first():
    _, _, V = _setup()
    P = 1
    kids = np.arange(B + 1, B + 33, dtype=np.int32)

    def scenario(eng):
        res = _solve(eng, np.zeros(B, np.int32), DST1, V)
        _keep(eng, [P])
        res += _solve(eng, np.full(32, P, np.int32), kids, V[:1] * np.linspace(0.9, 1.1, 32)[:, None] + 0.01)
        _keep(eng, kids)
        parked = eng.park_stats()["parked"]
        res += _solve(eng, np.zeros(4, np.int32), [P, 2, 3, 4], V[10:14])      # P is overwritten: its parked children still read it
        eng.discard_pending()
        res += _solve(eng, kids, np.arange(2 * B + 1, 2 * B + 33), V[:1] * np.linspace(1.1, 0.9, 32)[:, None] - 0.01)
        eng.discard_pending()
        return res, parked

    on, off = _both(scenario)
    ps = on[-2]
    print(ps, "parked before P was overwritten:", on[1])
    assert ps["forced"] > 0, ps
    assert ps["forced"] + ps["for_child"] == ps["parked"] and ps["live"] == 0, ps


def test_a_parked_slot_that_is_overwritten_or_reset_loses_its_record():
    _, _, V = _setup()

    def scenario(eng):
        res = _solve(eng, np.zeros(B, np.int32), DST1, V)
        _keep(eng, KEEP)
        res += _solve(eng, np.zeros(2, np.int32), KEEP[:2], V[50:52])          # two parked slots reused as dst
        _keep(eng, KEEP[:2])                                                   # (kept again: they start LPs below)
        eng.reset_slot(int(KEEP[2]))
        eng.drop_parked(KEEP[3:4])
        src = np.concatenate([KEEP[:3], KEEP[4:8]])
        res += _solve(eng, src, np.arange(B + 1, B + 1 + len(src)), V[20:20 + len(src)])
        eng.discard_pending()
        return (res,)

    on, off = _both(scenario)
    ps = on[-2]
    print(ps)
    assert ps["dropped"] > 0 and ps["for_child"] > 0, ps
    assert ps["live"] == ps["parked"] - ps["dropped"] - ps["for_child"] - ps["forced"], ps


def test_an_lp_that_has_passed_once_and_ends_with_pivots_pending():
    """more than KP = 6 pivots from the parent: the LP has written its slot once (flushed) and its parked pass works in place"""
    _, _, V = _setup()
    far = np.concatenate([V[::3] * 3.0 + 1.0, V[::3] * 0.3])
    src = np.concatenate([KEEP, KEEP])
    dst2 = np.arange(B + 1, B + 1 + len(src), dtype=np.int32)

    def scenario(eng):
        res = _solve(eng, np.zeros(B, np.int32), DST1, V)
        _keep(eng, KEEP)
        first = eng.park_stats()["parked"]
        res += _solve(eng, src, dst2, far)
        it = res[-5]
        _keep(eng, dst2)
        res += _solve(eng, dst2, np.arange(2 * B + 1, 2 * B + 1 + len(dst2)), far * 1.02)
        eng.discard_pending()
        return res, it, first

    on, off = _both(scenario)
    it = on[1]
    print("pivots of the second generation:", it.tolist())
    assert np.any(it > 6), it
    assert np.any((it > 6) & (it % 6 != 0)), it          # (ends with pivots pending after its pass)
    assert on[-2]["for_child"] > on[2] > 0, (on[-2], on[2])      # passes of the second generation's slots were parked and made


def test_materialise_reaches_a_slot_parked_two_batches_earlier():
    _, _, V = _setup()

    def scenario(eng):
        res = _solve(eng, np.zeros(B, np.int32), DST1, V)
        _keep(eng, KEEP)
        for k in range(2):
            res += _solve(eng, np.zeros(8, np.int32), np.arange(B + 1 + 8 * k, B + 9 + 8 * k), V[8 * k:8 * k + 8] * 1.01)
            eng.discard_pending()
        live = eng.park_stats()["live"]
        eng.materialise(KEEP[:5])
        live2 = eng.park_stats()["live"]
        eng.set_park(0)                                  # the slots are ordinary slots now: solved from with the engine of today
        res += _solve(eng, KEEP[:5], np.arange(2 * B + 1, 2 * B + 6), V[30:35])
        eng.discard_pending()
        return res, live, live2

    on, off = _both(scenario)
    assert 0 < on[1] - on[2] <= 5, on[1:3]            # (a slot that had passed and ended with nothing pending was never parked)


def test_the_fill_byte_of_fresh_memory_does_not_matter():
    """the store is fresh device memory, and a record holds only the rows of its pending pivots: the first case again on memory
    filled with 0x7F (BSLV_FILL is read once per process)"""
    env = dict(os.environ, BSLV_FILL="0x7F")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert "Memory access fault" not in p.stderr, p.stderr[-800:]
    assert p.returncode == 0, p.stderr[-1500:]
    row = json.loads(p.stdout.strip().splitlines()[-1])
    assert row["fill"] == "0x7F"
    assert row["sha256"] == _digest(_case1()[0][0]), row


if __name__ == "__main__":
    on, off = _case1()
    print(json.dumps(dict(fill=os.environ.get("BSLV_FILL", "0"), park=on[-2], sha256=_digest(on[0]))), flush=True)
