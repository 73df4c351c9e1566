"""GPU: canonical optimal duals of the LP engine (bslv_lpq_set_canonical, the tie phase of lp_engine.hip) against scipy's HiGHS.

P2(v) is primal degenerate where the ray v + z c meets an edge or a vertex of the upper image; every w of the normal cone is then
optimal and the engine returns the one its pivots reached.  With the switch on it has to return the dual of P2(v + t d) for small
t > 0 -- which HiGHS computes by solving the shifted LPs (tests/canonical_cases.py: the keep rule, the conditions on the case sets)
-- whatever basis the LP started from, and leave status and objective as they are bit for bit.  With the switch off nothing may
differ from an engine that never saw the new calls.

Wide sets (canonical_cases.WIDE: covering problems of 24 rows whose P2 has N columns), the threshold of the launch code each pair of
names straddles and the line of bensolve_amd/csrc/lp_engine.hip it comes from:
  wide-24x252x3  wide-24x253x3     N = 256, 257: one workgroup width of NT = 256 columns against a second stride of every
                                   "for (int j = tid; j < N; j += NT)" of tie_once (k_select_tie runs "dim3(plan.nt)" threads)
  wide-24x1116x3 wide-24x1117x3    N = 1120, 1121: the 1024-thread k_flush that makes the tie pivots' tableau pass: flush_launch,
                                   "big_flush = e ? atoi(e) > NT : lds > 53 * 1024" with lds = KP * ldt * 8, ldt = 1120 against 1136
  wide-24x1531x3 wide-24x1532x3    N = 1535, 1536: plan_select, "L.N >= 1536 ? NT_BIG : NT" -- k_select_tie's block size with it
  wide-24x2043x4 wide-24x2044x4    N = 2048, 2049: plan_init, "ld2 > 16 * WAVE": k_init_grouped against k_init
q = 3 gives P2 M + 1 = 32 rows, the last row tile of k_flush is full; q = 4 gives 34, that tile holds a single row.  Every wide set
has to show tie pivots, and the N = 1121 set gives the same bits under the other launch shapes (BSLV_FLUSH_NT, BSLV_SELECT_NT)."""
import os

import numpy as np
import pytest

import canonical_cases as cc
from bensolve_amd.lp import P2Model, LpEngine

pytestmark = pytest.mark.gpu
RTOL = 1e-9               # tests/test_lp_gpu.py's bound against HiGHS
NAMES = sorted(cc.PROBLEMS)
WIDE_NAMES = [cc.WIDE_NAMES[N] for N in sorted(cc.WIDE)]


def _solve_cold_then_batch(eng, model, V, canonical=False):
    """every LP from the optimal slot of the first one (slot 0), one batch.  The parent in slot 0 is solved with the switch off in
    every engine: "bit for bit" compares solves that start from the same basis."""
    B = len(V)
    ub = model.ub_for(V)
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), ub[:1])
    assert st0[0] == 4
    if canonical:
        assert eng.set_canonical(1, cc.direction(model.q) @ model.R) == 0 and eng.get_canonical() == 1
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.full((B, model.r), -np.inf), ub)
    return dst, st, it


def _off_and_on(name):
    """the switch-off solve and the switch-on solve of a case set, each on an engine of its own"""
    prob, c = cc.cases(name)
    cc.check_case_set(c)
    model = P2Model(prob)
    V = c["V"]
    out = {}
    for on in (0, 1):
        eng = LpEngine.from_model(model, pool_slots=len(V) + 2)
        dst, st, it = _solve_cold_then_batch(eng, model, V, canonical=bool(on))
        out[on] = dict(st=st.copy(), it=it.copy(), obj=eng.obj(dst), w=eng.dual(dst, model.w_first, model.q), y=eng.primal(dst, model.y_first, model.q),
                       canon=eng.last_canonical_stats())
        eng.close()
    return c, out


_results = {}


def _res(name):
    if name not in _results:
        _results[name] = _off_and_on(name)
    return _results[name]


@pytest.mark.parametrize("name", NAMES)
def test_switch_on_returns_the_dual_of_the_shifted_lp(name):
    c, out = _res(name)
    off, on = out[0], out[1]
    print("%s: %d cases, %d degenerate; off-solve differs from the canonical w in %d; tie phase %s" % (
        name, len(c["V"]), int(c["degenerate"].sum()), int((np.abs(off["w"] - c["w"]).max(axis=1) > 1e-6).sum()), on["canon"]))
    print("largest |w - expected| with the switch on: %.3e" % np.abs(on["w"] - c["w"]).max())
    assert np.all(off["st"] == 4)
    assert np.array_equal(on["st"], off["st"])
    assert on["obj"].tobytes() == off["obj"].tobytes(), "the objective changed with the switch: %s" % (on["obj"] - off["obj"])
    assert on["y"].tobytes() == off["y"].tobytes(), "primal values changed with the switch"      # (a tie pivot is a step of length zero)
    np.testing.assert_allclose(off["obj"], c["z"], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(on["w"], c["w"], rtol=RTOL, atol=1e-9)
    if name == "octahedron":
        N = cc.octahedron_normals()
        for w in on["w"]:
            assert np.abs(N - w).max(axis=1).min() <= 1e-9, w


@pytest.mark.parametrize("name", NAMES)
def test_the_counters_of_the_tie_phase_are_coherent(name):
    c, out = _res(name)
    off, on = out[0], out[1]
    moved = int((c["degenerate"] & (np.abs(off["w"] - c["w"]).max(axis=1) > 1e-6)).sum())     # degenerate cases whose off-solve gave another w
    print("%s: %d degenerate cases whose off-solve gave another w; %s" % (name, moved, on["canon"]))
    assert on["canon"]["entered"] >= moved and on["canon"]["tie_pivots"] >= moved
    assert on["canon"]["entered"] <= len(c["V"]) and on["canon"]["capped"] == 0
    assert off["canon"] == dict(entered=0, tie_pivots=0, no_candidate=0, capped=0)
    if name == "octahedron":
        assert moved > 0, "no case of the set shows the defect the switch is for"


@pytest.mark.parametrize("name", NAMES)
def test_result_does_not_depend_on_the_start(name):
    """the same cases warm-started from a solved SIBLING's slot (case k from the optimal slot of case k - 1, itself canonical),
    in one batch, with lazy tableaux on and the slots materialised afterwards"""
    c, out = _res(name)
    prob, _ = cc.cases(name)
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    eng = LpEngine.from_model(model, pool_slots=2 * B + 2)
    dst, st, _ = _solve_cold_then_batch(eng, model, V, canonical=True)
    assert np.all(st == 4)
    eng.set_lazy(1)
    dst2 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    st2, _ = eng.solve_batch(np.roll(dst, 1), dst2, np.full((B, model.r), -np.inf), model.ub_for(V))
    assert np.all(st2 == 4)
    w_lazy = eng.dual(dst2, model.w_first, model.q)
    obj_lazy = eng.obj(dst2)
    eng.materialise(dst2)
    eng.discard_pending()
    eng.set_lazy(0)
    w_mat = eng.dual(dst2, model.w_first, model.q)
    # the materialised slots are what later LPs start from: solved again in place they need no pivot and give the same dual
    st3, it3 = eng.solve_batch(dst2, dst2, np.full((B, model.r), -np.inf), model.ub_for(V))
    w_again = eng.dual(dst2, model.w_first, model.q)
    eng.close()
    print("%s: largest |w - expected| from a sibling's slot: %.3e" % (name, np.abs(w_lazy - c["w"]).max()))
    np.testing.assert_allclose(w_lazy, c["w"], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(obj_lazy, c["z"], rtol=RTOL, atol=1e-9)
    assert w_mat.tobytes() == w_lazy.tobytes()
    assert np.all(st3 == 4) and np.all(it3 == 0)
    np.testing.assert_allclose(w_again, c["w"], rtol=RTOL, atol=1e-9)


@pytest.mark.parametrize("name", NAMES)
def test_switch_off_is_the_engine_as_it_was(name):
    """duals, statuses, iteration counts and the counters of last_stats of an engine whose switch was set and cleared again equal
    those of an engine on which the new calls were never made, bit for bit"""
    c, out = _res(name)
    prob, _ = cc.cases(name)
    model = P2Model(prob)
    V = c["V"]
    rows = []
    for touched in (False, True):
        eng = LpEngine.from_model(model, pool_slots=len(V) + 2)
        if touched:
            assert eng.set_canonical(1, cc.direction(model.q) @ model.R) == 0
            assert eng.set_canonical(0) == 0 and eng.get_canonical() == 0
            eng.last_canonical_stats()
        dst, st, it = _solve_cold_then_batch(eng, model, V)
        ls = eng.last_stats()
        rows.append(dict(st=st.tobytes(), it=it.tobytes(), w=eng.dual(dst, 0, model.M + model.N).tobytes(), obj=eng.obj(dst).tobytes(),
                         x=eng.primal(dst, 0, model.M + model.N).tobytes(), stats={k: v for k, v in ls.items() if not k.endswith("_ms")}))
        eng.close()
    assert rows[0] == rows[1]
    assert rows[0]["st"] == out[0]["st"].tobytes() and rows[0]["it"] == out[0]["it"].tobytes()


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_tie_phase_pivots_on_the_wide_sets(name):
    """non-vacuity: at every width the tie phase really pivoted (the engine's answer is used to avoid an empty test, never as a bound)"""
    c, out = _res(name)
    on = out[1]
    print("lp_canonical_shapes %s: N %d, %d cases, %d degenerate, %d dropped; largest |w - expected| with the switch on %.3e; tie phase %s" % (
        name, P2Model(cc.cases(name)[0]).N, len(c["V"]), int(c["degenerate"].sum()), c["dropped"], np.abs(on["w"] - c["w"]).max(), on["canon"]))
    assert on["canon"]["tie_pivots"] > 0
    assert on["canon"]["entered"] == len(c["V"])          # (bslv_hip.h: all that ended OPTIMAL)


def test_launch_shapes_do_not_change_the_canonical_duals(monkeypatch):
    """the N = 1121 set under 256 and 1024 threads per k_flush workgroup and 1024 per selection (and tie) workgroup: status, pivots,
    objective, the full primal and dual vectors and the tie counters are the same bits as with nothing set; an engine of its own per arm"""
    name = cc.WIDE_NAMES[1121]
    prob, c = cc.cases(name)
    cc.check_case_set(c)
    model = P2Model(prob)
    assert model.N == 1121
    V, n = c["V"], model.M + model.N
    rows = []
    for env in ({}, {"BSLV_FLUSH_NT": "256"}, {"BSLV_FLUSH_NT": "1024"}, {"BSLV_SELECT_NT": "1024"}):
        for k in ("BSLV_SELECT_NT", "BSLV_FLUSH_NT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = LpEngine.from_model(model, pool_slots=len(V) + 2)
        dst, st, it = _solve_cold_then_batch(eng, model, V, canonical=True)
        rows.append(dict(st=st.tobytes(), it=it.tobytes(), obj=eng.obj(dst).tobytes(), x=eng.primal(dst, 0, n).tobytes(), y=eng.dual(dst, 0, n).tobytes(),
                         canon=eng.last_canonical_stats()))
        w = eng.dual(dst, model.w_first, model.q)
        eng.close()
        print("lp_canonical_shapes %s %s: largest |w - expected| %.3e; tie phase %s" % (name, env or "unset", np.abs(w - c["w"]).max(), rows[-1]["canon"]))
        np.testing.assert_allclose(w, c["w"], rtol=RTOL, atol=1e-9)
    assert rows[0]["canon"]["tie_pivots"] > 0
    for r in rows[1:]:
        assert r == rows[0]


def test_revised_form_refuses_the_switch():
    prob, c = cc.cases("octahedron")
    model = P2Model(prob)
    old = os.environ.get("BSLV_LP_REV")
    os.environ["BSLV_LP_REV"] = "1"
    try:
        eng = LpEngine.from_model(model, pool_slots=4)
    finally:
        if old is None:
            del os.environ["BSLV_LP_REV"]
        else:
            os.environ["BSLV_LP_REV"] = old
    try:
        assert eng.set_canonical(1, cc.direction(model.q)) == 2            # BSLV_E_ARG
        assert "revised" in eng.lib.bslv_last_error().decode()
        assert eng.get_canonical() == 0
        assert eng.set_canonical(0) == 0
    finally:
        eng.close()
