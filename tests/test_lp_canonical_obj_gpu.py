"""GPU: canonical optimal points of objective batches (bslv_lpq_set_canonical_obj, the tie phase k_select_tie_obj of lp_engine.hip).

The model is P1(w) as the dual variant builds it (canonical_obj_cases.P1Model); the chain is the feasibility LP in slot 0, an in-place
objective solve there with w = (1..1) / q and the switch off (PART 1 of dual_benson), then ONE batch of all kept weights of the problem
from slot 0.  The expected canonical y comes from HiGHS (canonical_obj_cases.build_cases); the bound on y and on the objectives is
tests/test_lp_gpu.py's against HiGHS, rtol 1e-9 with atol 1e-9.

Printed, not asserted: how many solves with the switch OFF end in a y that differs from the canonical one by more than 1e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest

import canonical_cases as cc
import canonical_obj_cases as co

pytestmark = pytest.mark.gpu
OPTIMAL = 4
RTOL = ATOL = 1e-9
ALL = co.COVERING + co.DECOYS
ZERO = dict(entered=0, tie_iters=0, unbounded=0, capped=0)


def _start(model, slots, lazy=False):
    """engine with the feasibility LP and PART 1's in-place solve (switch off) in slot 0"""
    eng = model.engine(slots)
    if lazy:
        eng.set_lazy(1)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
    assert st[0] == OPTIMAL, st
    st, _ = eng.solve_batch_obj([0], [0], model.y_first, np.full((1, model.q), 1.0 / model.q))
    assert st[0] == OPTIMAL, st
    assert eng.last_canonical_obj_stats() == ZERO
    return eng


def _batch(eng, model, W, src=None, dst=None):
    B = len(W)
    src = np.zeros(B, np.int32) if src is None else np.asarray(src, np.int32)
    dst = np.arange(1, B + 1, dtype=np.int32) if dst is None else np.asarray(dst, np.int32)
    st, it = eng.solve_batch_obj(src, dst, model.y_first, W)
    return dst, st, it


_runs = {}


def _run(name):
    """the chain with the switch off and on, once per problem: statuses, iterations, objectives, y, all values and duals, counters"""
    if name not in _runs:
        prob, c = co.cases(name)
        model = co.P1Model(prob)
        out = {}
        for on in (0, 1):
            eng = _start(model, len(c["W"]) + 1)
            if on:
                assert eng.set_canonical_obj(1, model.y_first, cc.direction(model.q)) == 0
                assert eng.get_canonical_obj() == 1
            dst, st, it = _batch(eng, model, c["W"])
            out[on] = dict(st=st, it=it, obj=eng.obj(dst), y=eng.primal(dst, model.y_first, model.q), val=eng.primal(dst, 0, model.M + model.N),
                           dual=eng.dual(dst, 0, model.M + model.N), stats=eng.last_canonical_obj_stats(), last=eng.last_stats())
            eng.close()
        _runs[name] = (prob, c, model, out)
    return _runs[name]


def _off_differs(c, off):
    return np.abs(off["y"] - c["y"]).max(axis=1) > 1e-6


@pytest.mark.parametrize("name", ALL)
def test_off_and_on(name):
    prob, c, model, out = _run(name)
    off, on = out[0], out[1]
    assert np.all(off["st"] == OPTIMAL) and np.all(on["st"] == OPTIMAL), (off["st"], on["st"])
    differ = int(_off_differs(c, off).sum())
    print("%s: %d cases, %d degenerate; y of the switch-off solve differs from the canonical y by more than 1e-6 in %d; tie phase %s"
          % (name, len(c["W"]), int(c["degenerate"].sum()), differ, on["stats"]))
    print("   largest |y_on - y_expected| / (1 + |y|): %.3e" % (np.abs(on["y"] - c["y"]) / (1.0 + np.abs(c["y"]))).max())
    np.testing.assert_allclose(on["obj"], off["obj"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(off["obj"], c["z"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(on["obj"], c["z"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(on["y"], c["y"], rtol=RTOL, atol=ATOL)
    if name in co.DECOYS:
        V = co.decoy_vertices(model.q)
        for y in on["y"]:
            assert np.abs(V - y).max(axis=1).min() <= 1e-9, y


@pytest.mark.parametrize("name", ALL)
def test_counters(name):
    prob, c, model, out = _run(name)
    off, on = out[0], out[1]
    s = on["stats"]
    assert 0 < s["entered"] <= len(c["W"])
    assert s["tie_iters"] >= int((c["degenerate"] & _off_differs(c, off)).sum())
    assert s["capped"] == 0 and s["unbounded"] == 0
    assert off["stats"] == ZERO
    assert int(on["it"].sum()) - int(off["it"].sum()) == s["tie_iters"]      # tie iterations are counted in iters[]


@pytest.mark.parametrize("name", ALL)
def test_the_start_does_not_matter(name):
    """case k from the canonical slot of case k - 1, lazy tableaux on; then in place on the materialised slots: no iteration"""
    prob, c, model, out = _run(name)
    W = c["W"]
    B = len(W)
    eng = _start(model, 2 * B + 1, lazy=True)
    try:
        assert eng.set_canonical_obj(1, model.y_first, cc.direction(model.q)) == 0
        dst, st, _ = _batch(eng, model, W)
        assert np.all(st == OPTIMAL)
        dst2 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
        _, st, _ = _batch(eng, model, W, src=np.roll(dst, 1), dst=dst2)
        assert np.all(st == OPTIMAL)
        eng.materialise(dst2)
        y2 = eng.primal(dst2, model.y_first, model.q)
        np.testing.assert_allclose(y2, c["y"], rtol=RTOL, atol=ATOL)
        _, st, it = _batch(eng, model, W, src=dst2, dst=dst2)
        assert np.all(st == OPTIMAL)
        assert np.all(it == 0), it
        assert eng.last_canonical_obj_stats()["tie_iters"] == 0
        np.testing.assert_allclose(eng.primal(dst2, model.y_first, model.q), c["y"], rtol=RTOL, atol=ATOL)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ALL)
def test_switch_off_is_the_engine_as_it_was(name):
    """an engine whose switch was set and cleared against one that never saw the calls: bit for bit"""
    prob, c, model, out = _run(name)
    rows = []
    for touched in (True, False):
        eng = _start(model, len(c["W"]) + 1)
        if touched:
            assert eng.set_canonical_obj(1, model.y_first, cc.direction(model.q)) == 0
            assert eng.set_canonical_obj(0) == 0
            assert eng.get_canonical_obj() == 0
        dst, st, it = _batch(eng, model, c["W"])
        ls = eng.last_stats()
        rows.append(dict(st=st.tobytes(), it=it.tobytes(), x=eng.primal(dst, 0, model.M + model.N).tobytes(), d=eng.dual(dst, 0, model.M + model.N).tobytes(),
                         obj=eng.obj(dst).tobytes(), stats={k: v for k, v in ls.items() if not k.endswith("_ms")}))
        if touched:
            assert eng.last_canonical_obj_stats() == ZERO
        eng.close()
    assert rows[0] == rows[1]
    off = out[0]
    assert rows[0]["st"] == off["st"].tobytes() and rows[0]["it"] == off["it"].tobytes() and rows[0]["x"] == off["val"].tobytes()


def test_the_two_tie_phases_keep_their_own_counters():
    """both switches on in one engine, on the smallest model (decoy-3: 4 rows, 10 columns): an objective batch leaves the counters of
    the canonical basis at zero, a solve_batch leaves those of the objective phase standing (only an objective batch resets them), and
    the same objective batch again gives the same counters and the same solutions, bit for bit"""
    prob, c, model, _ = _run("decoy-3")
    W = c["W"]
    B = len(W)
    eng = _start(model, 2 * B + 1)
    try:
        assert eng.set_canonical_obj(1, model.y_first, cc.direction(model.q)) == 0
        assert eng.set_canonical(1, np.ones(eng.vcnt)) == 0
        assert eng.get_canonical_obj() == 1 and eng.get_canonical() == 1
        zero = dict(entered=0, tie_pivots=0, no_candidate=0, capped=0)

        def batch(dst):
            _, st, _ = _batch(eng, model, W, dst=dst)
            assert np.all(st == OPTIMAL), st
            n = model.M + model.N
            return eng.last_canonical_obj_stats(), [eng.obj(dst).tobytes(), eng.primal(dst, 0, n).tobytes(), eng.dual(dst, 0, n).tobytes()]

        dst = np.arange(1, B + 1, dtype=np.int32)
        stats, first = batch(dst)
        assert stats["entered"] > 0, stats
        assert eng.last_canonical_stats() == zero
        st, _ = eng.solve_batch(dst[:1], dst[:1], np.zeros((1, 0)), np.zeros((1, 0)))
        assert st[0] == OPTIMAL, st
        assert eng.last_canonical_obj_stats() == stats
        assert eng.last_canonical_stats() == zero
        stats2, second = batch(np.arange(B + 1, 2 * B + 1, dtype=np.int32))
        assert stats2 == stats
        assert second == first
    finally:
        eng.close()


def _check_certificates(model, prob, val, dual, W, obj):
    """_check_certificates of tests/test_lp_rev_obj_gpu.py: y = P x, x feasible; the duals of the rows and the reduced costs of the
    columns have the signs their bounds allow, sit only on variables at a bound, and give the objective back.

    One line differs from the original, and the test says why.  The original accepts a dual of the wrong sign up to tol = 1e-9 and then
    takes the bound of the strong-duality sum from the SIGN of every dual beyond 1e-12 -- for a wrong-signed dual in (1e-12, 1e-9] that
    is the infinite side of a variable it has just accepted, and `isfinite(bound)` fails.  Its own weights are generic and never meet
    that window.  The weights here are facet normals rounded to 12 digits, so reduced costs of 1e-12 are what a tie looks like: on an
    MI355X the UNCHANGED engine (switch off) returns 5 such duals on covering-40x20x4 (largest 2.4e-12, on a cover row that sits on its
    lower bound 1 with a dual of -1.9e-12), the switch on 6 there and 1 on covering-30x80x3 (2.0e-12).  Such a dual takes the bound its
    variable sits on; every assertion of the original stays, at its tolerance, and the sum now includes those terms."""
    M, n = model.M, model.n
    x, y = val[:, M:M + n], val[:, model.y_first:]
    np.testing.assert_allclose(x @ prob["P"].T, y, rtol=0, atol=1e-8)
    assert np.all(x >= -1e-9) and np.all(x @ prob["A"].T >= 1 - 1e-8)
    np.testing.assert_allclose(np.einsum("bk,bk->b", W, y), obj, rtol=1e-9, atol=1e-9)
    lo, up = model.lo[None, :], model.up[None, :]
    at_lo = np.abs(val - lo) <= 1e-8 * (1 + np.abs(np.where(np.isinf(lo), 0, lo)))
    at_up = np.abs(val - up) <= 1e-8 * (1 + np.abs(np.where(np.isinf(up), 0, up)))
    fixed = (lo == up) & np.ones_like(val, bool)
    tol = 1e-9
    assert np.all(fixed | (dual <= tol) | at_lo), "positive dual on a variable off its lower bound"
    assert np.all(fixed | (dual >= -tol) | at_up), "negative dual on a variable off its upper bound"
    bound = np.where(dual > 0, np.broadcast_to(lo, val.shape), np.broadcast_to(up, val.shape))
    bound = np.where(fixed, np.broadcast_to(lo, val.shape), bound)
    bound = np.where(np.abs(dual) <= 1e-12, 0.0, bound)
    small = np.isinf(bound) & (np.abs(dual) <= tol)       # accepted above although its sign is wrong: the bound it sits on
    bound = np.where(small & at_lo, np.broadcast_to(lo, val.shape), np.where(small & at_up, np.broadcast_to(up, val.shape), bound))
    assert np.all(np.isfinite(bound))
    np.testing.assert_allclose((dual * bound).sum(axis=1), obj, rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("name", ALL)
def test_certificates(name):
    prob, c, model, out = _run(name)
    for r in (out[0], out[1]):                     # the same check holds for the engine as it was
        _check_certificates(model, prob, r["val"], r["dual"], c["W"], r["obj"])


def test_refusals(monkeypatch):
    prob, c = co.cases("decoy-3")
    model = co.P1Model(prob)
    d = cc.direction(model.q)
    eng = _start(model, len(c["W"]) + 1)
    try:
        st, it = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
        before = (int(st[0]), int(it[0]))
        assert before[0] == OPTIMAL
        bad = d.copy(); bad[1] = np.nan
        assert eng.set_canonical_obj(1, model.y_first, bad) == 2 and eng.get_canonical_obj() == 0          # BSLV_E_ARG
        bad[1] = np.inf
        assert eng.set_canonical_obj(1, model.y_first, bad) == 2
        assert eng.set_canonical_obj(1, model.y_first, None) == 2
        assert eng.set_canonical_obj(1, model.M + model.N - 1, d) == 2 and eng.set_canonical_obj(1, -1, d) == 2      # bad ranges
        assert eng.get_canonical_obj() == 0
        assert eng.set_canonical_obj(1, model.y_first, d) == 0
        # a batch over another cost range is refused while the switch is on ...
        with pytest.raises(Exception, match="cost range"):
            eng.solve_batch_obj([0], [1], model.y_first + 1, np.ones((1, model.q - 1)))
        with pytest.raises(Exception, match="cost range"):
            eng.solve_batch_obj([0], [1], model.y_first, np.ones((1, model.q - 1)))
        # ... solve_batch does not know the switch: what it answered before the switch was set
        st, it = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
        assert (int(st[0]), int(it[0])) == before
        # ... and it is independent of bslv_lpq_set_canonical
        assert eng.get_canonical() == 0
        dst, st, _ = _batch(eng, model, c["W"])
        assert np.all(st == OPTIMAL)
        np.testing.assert_allclose(eng.primal(dst, model.y_first, model.q), c["y"], rtol=RTOL, atol=ATOL)
    finally:
        eng.close()
    monkeypatch.setenv("BSLV_LP_REV", "1")
    eng = model.engine(4)
    try:
        assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
        assert eng.set_canonical_obj(1, model.y_first, d) == 2
        assert "revised" in eng.lib.bslv_last_error().decode()
        assert eng.get_canonical_obj() == 0 and eng.set_canonical_obj(0) == 0
    finally:
        eng.close()


_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import canonical_cases as cc, canonical_obj_cases as co
import test_lp_canonical_obj_gpu as t
prob, c = co.cases("covering-30x80x3")
model = co.P1Model(prob)
eng = t._start(model, len(c["W"]) + 1)
assert eng.set_canonical_obj(1, model.y_first, cc.direction(model.q)) == 0
dst, st, it = t._batch(eng, model, c["W"])
assert np.all(st == 4)
print("SHA", hashlib.sha256(np.ascontiguousarray(eng.primal(dst, model.y_first, model.q)).tobytes()).hexdigest(), eng.last_canonical_obj_stats()["tie_iters"])
eng.close()
"""


def test_fill_byte():
    """fresh device memory filled with 0x7F instead of zeros: the same y, bit for bit (the phase reads nothing it has not written)"""
    here = os.path.dirname(os.path.abspath(__file__))
    got = []
    for fill in (None, "0x7F"):
        env = {k: v for k, v in os.environ.items() if k != "BSLV_FILL"}
        if fill:
            env["BSLV_FILL"] = fill
        r = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got.append([l for l in r.stdout.splitlines() if l.startswith("SHA")][0])
    print(got)
    assert got[0] == got[1] and int(got[0].split()[2]) > 0
