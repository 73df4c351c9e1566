"""GPU: canonical optimal duals PER CALL (bslv_lpq_solve_batch_canonical), in the revised form above all -- its tie phase is
k_select_tie_rev / tie_once<true> of bensolve_amd/csrc/lp_engine.hip, and this call is the only way to it.

Expected duals are tests/canonical_cases.py's and tests/canonical_general_cases.py's (HiGHS on the shifted LPs, nothing from the code
under test); the bounds are tests/test_lp_canonical_gpu.py's, RTOL = 1e-9 with atol 1e-9.  The revised form is forced with
BSLV_LP_REV=1 at create and asserted with bslv_lpq_is_revised.

P2 sets: the three of canonical_cases.PROBLEMS and two pairs of wide ones -- N = 1535 / 1536, from where a selection (and the tie
kernel with it) runs NT_BIG threads and helper workgroups are possible at all, and N = 2048 / 2049, where ld goes 2048 -> 2064 and
"(L.ld + 2047) / 2048" 1 -> 2: the first shape with a helper workgroup.  The protocol is test_lp_canonical_gpu._solve_cold_then_batch's:
the parent cold into slot 0 by plain solve_batch, the kept LPs from slot 0 in one batch, once by solve_batch and once by the new call,
each on an engine of its own.

Run as a script it is the child of three tests (the environment is read once per process): `helpers V.npy`, `fill` and `drift V.npy`
each print one JSON line."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import canonical_cases as cc
import canonical_general_cases as cg
from bensolve_amd._lib import BslvError
from bensolve_amd.lp import P2Model, LpEngine
from lp_cases import OPTIMAL, NLP
from test_lp_general_gpu import _engine, _env, _same_bits

pytestmark = pytest.mark.gpu
RTOL = 1e-9               # tests/test_lp_canonical_gpu.py's bound against HiGHS
E_ARG = 2
ZERO = dict(entered=0, tie_pivots=0, no_candidate=0, capped=0)
P2_NAMES = ["octahedron", "covering-40x20x4", "covering-30x80x3"] + [cc.WIDE_NAMES[N] for N in (1535, 1536, 2048, 2049)]
GENERAL = [(M, N, arr) for M, N in cg.SHAPES for arr in ("a", "b")]


def _p2_engine(model, slots, form="revised"):
    with _env(BSLV_LP_REV="1" if form == "revised" else None):
        eng = LpEngine.from_model(model, pool_slots=slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(form == "revised")
    return eng


def _dir(model):
    return cc.direction(model.q) @ model.R


def _cold_then_batch(eng, model, V, canonical):
    """test_lp_canonical_gpu._solve_cold_then_batch with the new call in place of the switch: the parent in slot 0 by plain solve_batch"""
    B = len(V)
    ub = model.ub_for(V)
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), ub[:1])
    assert st0[0] == OPTIMAL
    dst = np.arange(1, B + 1, dtype=np.int32)
    lo = np.full((B, model.r), -np.inf)
    if canonical:
        st, it = eng.solve_batch_canonical(_dir(model), np.zeros(B, np.int32), dst, lo, ub)
    else:
        st, it = eng.solve_batch(np.zeros(B, np.int32), dst, lo, ub)
    return dst, st, it


def _read_p2(eng, model, dst, st, it):
    n = model.M + model.N
    return dict(st=st.copy(), it=it.copy(), obj=eng.obj(dst), w=eng.dual(dst, model.w_first, model.q), y=eng.primal(dst, model.y_first, model.q),
                prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n), canon=eng.last_canonical_stats(),
                stats={k: v for k, v in eng.last_stats().items() if not k.endswith("_ms")})


_P2 = {}


def _p2(name):
    """the plain solve and the new call of a case set on revised engines, once"""
    if name not in _P2:
        prob, c = cc.cases(name)
        cc.check_case_set(c)
        model = P2Model(prob)
        out = {}
        for on in (0, 1):
            eng = _p2_engine(model, len(c["V"]) + 2)
            dst, st, it = _cold_then_batch(eng, model, c["V"], bool(on))
            out[on] = _read_p2(eng, model, dst, st, it)
            out[on]["get"] = eng.get_canonical()
            eng.close()
        _P2[name] = (c, out)
    return _P2[name]


# ---- 1. the P2 sets on a revised engine -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P2_NAMES)
def test_the_call_returns_the_dual_of_the_shifted_lp(name):
    c, out = _p2(name)
    off, on = out[0], out[1]
    moved = int((c["degenerate"] & (np.abs(off["w"] - c["w"]).max(axis=1) > 1e-6)).sum())     # degenerate cases whose plain solve gave another w
    print("lp_rev_canonical %s: %d cases, %d degenerate, %d moved; largest |w - expected| by the call %.3e; tie phase %s; tie pivots per LP %s" % (
        name, len(c["V"]), int(c["degenerate"].sum()), moved, np.abs(on["w"] - c["w"]).max(), on["canon"], (on["it"] - off["it"]).tolist()))
    assert np.array_equal(on["st"], off["st"])
    assert _same_bits(on["obj"], off["obj"]), "the objective changed with the call: %s" % (on["obj"] - off["obj"])
    assert _same_bits(on["y"], off["y"]), "primal values changed with the call"      # (a tie pivot is a step of length zero)
    np.testing.assert_allclose(on["w"], c["w"], rtol=RTOL, atol=1e-9)
    assert on["canon"]["entered"] >= moved and on["canon"]["entered"] <= len(c["V"])
    assert on["canon"]["tie_pivots"] >= moved
    assert on["canon"]["capped"] == 0
    assert off["canon"] == ZERO
    assert on["get"] == 0 and off["get"] == 0
    if name == "octahedron":
        assert moved > 0, "no case of the set shows the defect the call is for"


def test_some_lp_makes_two_tie_pivots_in_one_launch():
    """its second pivot sees the first as a pending step: in g's entry it does not (that is built once), but in the pivot row's rho,
    in the tableau row and in the entering column it does.  Read from iters minus the plain solve's iters: an LP's tie pivots are made
    KP to a launch, so two of them lie in one"""
    most = {}
    for name in P2_NAMES:
        c, out = _p2(name)
        ok = (out[0]["st"] == OPTIMAL) & (out[1]["st"] == OPTIMAL)
        most[name] = int((out[1]["it"] - out[0]["it"])[ok].max())
    print("lp_rev_canonical most tie pivots of one LP: %s" % most)
    assert max(most.values()) >= 2, most


# ---- 2. start independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P2_NAMES)
def test_result_does_not_depend_on_the_start(name):
    """the same cases warm-started from a solved SIBLING's slot (case k from the optimal slot of case k - 1, itself canonical), in one
    batch with lazy tableaux on -- the phase then starts on pending pivots -- and the slots materialised afterwards; solved again in
    place by the new call they need no pivot"""
    prob, c = cc.cases(name)
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    lo, ub, d = np.full((B, model.r), -np.inf), model.ub_for(V), _dir(model)
    eng = _p2_engine(model, 2 * B + 2)
    dst, st, _ = _cold_then_batch(eng, model, V, True)
    assert np.all(st == OPTIMAL)
    eng.set_lazy(1)
    dst2 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    st2, _ = eng.solve_batch_canonical(d, np.roll(dst, 1), dst2, lo, ub)
    assert np.all(st2 == OPTIMAL)
    w_lazy = eng.dual(dst2, model.w_first, model.q)
    obj_lazy = eng.obj(dst2)
    eng.materialise(dst2)
    eng.discard_pending()
    eng.set_lazy(0)
    w_mat = eng.dual(dst2, model.w_first, model.q)
    st3, it3 = eng.solve_batch_canonical(d, dst2, dst2, lo, ub)
    w_again = eng.dual(dst2, model.w_first, model.q)
    eng.close()
    print("lp_rev_canonical %s: largest |w - expected| from a sibling's slot: %.3e" % (name, np.abs(w_lazy - c["w"]).max()))
    np.testing.assert_allclose(w_lazy, c["w"], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(obj_lazy, c["z"], rtol=RTOL, atol=1e-9)
    assert w_mat.tobytes() == w_lazy.tobytes()
    assert np.all(st3 == OPTIMAL) and np.all(it3 == 0), it3
    np.testing.assert_allclose(w_again, c["w"], rtol=RTOL, atol=1e-9)


# ---- 3. helpers do not show ---------------------------------------------------------------------------------------------------------------
def _wide_model(N):
    from bensolve_amd import synth
    n, q, seed = cc.WIDE[N][:3]
    return P2Model(synth.covering_vlp(24, n, q, seed))


def _child_batch(model, V):
    """the new call on a revised engine, as one JSON-able record of bits"""
    eng = _p2_engine(model, len(V) + 2)
    dst, st, it = _cold_then_batch(eng, model, V, True)
    rec = _read_p2(eng, model, dst, st, it)
    eng.close()
    return dict(st=rec["st"].tolist(), it=rec["it"].tolist(), obj=rec["obj"].tobytes().hex(), dual=hashlib.sha256(rec["dual"].tobytes()).hexdigest(),
                w=rec["w"].tobytes().hex(), canon=rec["canon"])


def _spawn(args, env, timeout=240):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert "Memory access fault" not in p.stderr, "%s: %s" % (args, p.stderr[-800:])
    assert p.returncode == 0, "%s: rc %d\n%s" % (args, p.returncode, p.stderr[-1500:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_helpers_do_not_change_a_bit(tmp_path):
    """N = 2049 with one workgroup per LP (BSLV_REV_HELPERS=1) and with the default, a helper beside it: duals, objective and
    iteration counts are the same bits.  The variable is read once per process: a child each (the first that fails ends the test)"""
    c, out = _p2(cc.WIDE_NAMES[2049])
    vfile = str(tmp_path / "V.npy")
    np.save(vfile, c["V"])
    rows = []
    for helpers in ("1", None):
        env = dict(os.environ)
        env.pop("BSLV_REV_HELPERS", None)
        if helpers:
            env["BSLV_REV_HELPERS"] = helpers
        rows.append(_spawn(["helpers", vfile], env))
    assert rows[0] == rows[1]
    assert rows[1]["canon"]["tie_pivots"] > 0
    assert rows[1]["w"] == out[1]["w"].tobytes().hex() and rows[1]["it"] == out[1]["it"].tolist()


# ---- 4. general models ------------------------------------------------------------------------------------------------------------------
def _general_start(c, slots):
    eng = _engine(c["A"], c["lo"], c["up"], c["cost"], c["var_first"], c["var_cnt"], slots, "revised")
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], c["vlo0"][None], c["vup0"][None])
    assert st0[0] == OPTIMAL
    return eng


def _read(eng, dst, st, it):
    n = eng.M + eng.N
    return dict(st=np.array(st), it=np.array(it), obj=eng.obj(dst), prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n), canon=eng.last_canonical_stats())


def _general_off_on(c, B):
    dst = np.arange(1, B + 1, dtype=np.int32)
    rec = {}
    for on in (0, 1):
        eng = _general_start(c, B + 1)
        if on:
            st, it = eng.solve_batch_canonical(c["dir"], np.zeros(B, np.int32), dst, c["vlo"], c["vup"])
        else:
            st, it = eng.solve_batch(np.zeros(B, np.int32), dst, c["vlo"], c["vup"])
        rec[on] = _read(eng, dst, st, it)
        eng.close()
    return rec[0], rec[1]


@pytest.mark.parametrize("M,N,arr", GENERAL)
def test_general_models_reach_the_expected_full_dual(oracle, M, N, arr):
    """`below`, a tied basic per-LP variable's own shift, a per-LP column entering, the NS_F skip; arrangement "a" has a row range,
    "b" a column range, for the combined column of the entry"""
    c = cg.tied_set(M, N, arr)
    cg.check_tied_set(c)
    off, on = _general_off_on(c, len(c["lps"]))
    moved = int((c["degenerate"] & (np.abs(off["dual"] - c["dual"]).max(axis=1) > 1e-6)).sum())
    print("lp_rev_canonical general M %d N %d arr %s: %d cases, %d moved; largest |dual - expected| by the call %.3e; tie phase %s" % (
        M, N, arr, len(c["lps"]), moved, np.abs(on["dual"] - c["dual"]).max(), on["canon"]))
    assert np.all(off["st"] == OPTIMAL) and np.array_equal(on["st"], off["st"])
    assert _same_bits(on["obj"], off["obj"]) and _same_bits(on["prim"], off["prim"])
    np.testing.assert_allclose(on["dual"], c["dual"], rtol=RTOL, atol=1e-9)
    assert moved <= on["canon"]["entered"] <= len(c["lps"])
    assert on["canon"]["capped"] == 0 and off["canon"] == ZERO


@pytest.mark.parametrize("M,N", cg.EXIT_SHAPES)
def test_exit_without_an_entering_candidate(oracle, M, N):
    e = cg.exit_set(M, N)
    off, on = _general_off_on(e, NLP)
    opt = e["optimal"]
    print("lp_rev_canonical exit M %d N %d: %d OPTIMAL LPs of %d; tie phase %s" % (M, N, int(opt.sum()), NLP, on["canon"]))
    assert np.array_equal(on["st"], off["st"]) and np.array_equal(on["st"] == OPTIMAL, opt)
    assert _same_bits(on["obj"][opt], off["obj"][opt]) and _same_bits(on["prim"][opt], off["prim"][opt])
    np.testing.assert_allclose(on["obj"][opt], e["z"][opt], rtol=RTOL, atol=1e-9)
    assert on["canon"]["capped"] == 0
    assert on["canon"]["entered"] == int(opt.sum())
    assert on["canon"]["no_candidate"] == int(opt.sum()), on["canon"]


# ---- 5. the call leaves no trace; arguments ---------------------------------------------------------------------------------------------
def _next_plain(eng, model, V):
    """a plain solve_batch of every case from the parent slot 0 into fresh slots"""
    B = len(V)
    dst = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.full((B, model.r), -np.inf), model.ub_for(V))
    return _read_p2(eng, model, dst, st, it)


def test_the_call_leaves_no_trace():
    prob, c = cc.cases("covering-40x20x4")
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    rows = []
    for called in (True, False):
        eng = _p2_engine(model, 2 * B + 2)
        _cold_then_batch(eng, model, V, called)
        rows.append(_next_plain(eng, model, V))
        assert eng.get_canonical() == 0
        assert eng.set_canonical(1, _dir(model)) == E_ARG and "revised" in eng.lib.bslv_last_error().decode()
        assert eng.get_canonical() == 0
        eng.close()
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(rows[0][k], rows[1][k]), k
    assert rows[0]["stats"] == rows[1]["stats"] and rows[0]["canon"] == rows[1]["canon"] == ZERO


@pytest.mark.parametrize("form", ["revised", "tableau"])
def test_bad_arguments_change_nothing(form):
    """dir = NULL and a NaN in dir: BSLV_E_ARG, and the next solve is the same bits as on an engine that never saw the bad calls"""
    prob, c = cc.cases("octahedron")
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    lo, ub = np.full((B, model.r), -np.inf), model.ub_for(V)
    rows = []
    for bad in (True, False):
        eng = _p2_engine(model, 2 * B + 2, form)
        _cold_then_batch(eng, model, V, False)
        if bad:
            nan = _dir(model).copy()
            nan[-1] = np.nan
            for d in (None, nan):
                with pytest.raises(BslvError, match="error 2"):
                    eng.solve_batch_canonical(d, np.zeros(B, np.int32), np.arange(1, B + 1, dtype=np.int32), lo, ub)
            eng.lib.bslv_lpq_solve_batch_canonical.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 6
            assert eng.lib.bslv_lpq_solve_batch_canonical(None, None, 0, None, None, None, None, None, None) == E_ARG
        rows.append(_next_plain(eng, model, V))
        eng.close()
    for k in ("st", "it", "obj", "prim", "dual"):
        assert _same_bits(rows[0][k], rows[1][k]), k
    assert rows[0]["stats"] == rows[1]["stats"] and rows[0]["canon"] == rows[1]["canon"]


# ---- 6. tableau form: the call IS set_canonical(1, dir); solve_batch; the old switch back -------------------------------------------------
def _all_last(eng):
    return dict(stats={k: v for k, v in eng.last_stats().items() if not k.endswith("_ms")}, canon=eng.last_canonical_stats(),
                pricing=eng.last_pricing_stats(), ppricing=eng.last_primal_pricing_stats(), ray=eng.last_ray_stats())


@pytest.mark.parametrize("name", ["octahedron", "covering-30x80x3"])
@pytest.mark.parametrize("switch", ["off", "other"])
def test_tableau_form_the_call_is_the_switch_for_one_batch(name, switch):
    """twin engines in the tableau form, once with the engine's switch off and once with it on for ANOTHER direction -- which a
    following plain solve_batch must still use"""
    prob, c = cc.cases(name)
    model = P2Model(prob)
    V, B = c["V"], len(c["V"])
    lo, ub, d = np.full((B, model.r), -np.inf), model.ub_for(V), _dir(model)
    other = d[::-1].copy() * np.array([1.0 + 0.25 * j for j in range(len(d))])
    src, dst = np.zeros(B, np.int32), np.arange(1, B + 1, dtype=np.int32)
    rows = []
    for by_call in (True, False):
        eng = _p2_engine(model, 2 * B + 2, "tableau")
        _cold_then_batch(eng, model, V[:1], False)
        if switch == "other":
            assert eng.set_canonical(1, other) == 0
        if by_call:
            st, it = eng.solve_batch_canonical(d, src, dst, lo, ub)
        else:
            assert eng.set_canonical(1, d) == 0
            st, it = eng.solve_batch(src, dst, lo, ub)
            assert eng.set_canonical(1, other) == 0 if switch == "other" else eng.set_canonical(0) == 0
        assert eng.get_canonical() == int(switch == "other")
        rec = dict(_read_p2(eng, model, dst, st, it), last=_all_last(eng))
        nxt = _next_plain(eng, model, V)
        rec.update({"next_" + k: v for k, v in nxt.items()}, next_last=_all_last(eng))
        eng.close()
        rows.append(rec)
    a, b = rows
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert _same_bits(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    np.testing.assert_allclose(a["w"], c["w"], rtol=RTOL, atol=1e-9)
    assert a["canon"]["tie_pivots"] > 0
    if switch == "off":
        assert a["next_canon"] == ZERO
    else:
        assert a["next_canon"]["entered"] == B      # (the engine's own switch and direction are in force again)


# ---- 7. the drift hook reaches a tie pivot ------------------------------------------------------------------------------------------------
def test_a_tie_pivot_that_fails_the_cross_check_keeps_the_optimum(tmp_path):
    """BSLV_LP_REV_DRIFT=b:p with p = the plain solve's iters[b] + 1: the first tie pivot of LP b.  Nothing is committed, the LP stays
    OPTIMAL with the same objective bits on the basis the solve had reached and counts in stats[3]; every other LP is as without the hook"""
    name = "octahedron"
    c, out = _p2(name)
    off, on = out[0], out[1]
    tied = np.nonzero((on["it"] > off["it"]) & (on["st"] == OPTIMAL))[0]
    tied = tied[tied > 0]          # (the hook names an LP by its index in a batch, and the parent's cold solve is LP 0 of its own)
    assert len(tied) > 0
    b = int(tied[0])
    vfile = str(tmp_path / "V.npy")
    np.save(vfile, c["V"])
    env = dict(os.environ, BSLV_LP_REV_DRIFT="%d:%d" % (b, int(off["it"][b]) + 1), BSLV_CASES=name)
    row = _spawn(["drift", vfile], env)
    st, it = np.array(row["st"]), np.array(row["it"])
    w = np.frombuffer(bytes.fromhex(row["w"])).reshape(-1, on["w"].shape[1])
    obj = np.frombuffer(bytes.fromhex(row["obj"]))
    print("lp_rev_canonical drift: LP %d at pivot %d; tie phase %s" % (b, int(off["it"][b]) + 1, row["canon"]))
    assert st[b] == OPTIMAL and obj[b].tobytes() == off["obj"][b].tobytes()
    assert it[b] == off["it"][b] and w[b].tobytes() == off["w"][b].tobytes()      # (the basis the plain solve ends in)
    assert row["canon"]["capped"] == 1
    others = np.arange(len(st)) != b
    assert np.array_equal(st[others], on["st"][others]) and np.array_equal(it[others], on["it"][others])
    assert w[others].tobytes() == on["w"][others].tobytes() and obj[others].tobytes() == on["obj"][others].tobytes()


# ---- 8. poisoned allocations ------------------------------------------------------------------------------------------------------------
def test_the_call_does_not_depend_on_the_fill_byte(tmp_path):
    """the project's standing guard for a kernel that reads a word nobody wrote (test_lp_rev_primal_gpu's pattern): covering-40x20x4
    under two fill bytes of the engine's allocations, a child each"""
    c, out = _p2("covering-40x20x4")
    vfile = str(tmp_path / "V.npy")
    np.save(vfile, c["V"])
    rows = []
    for fill in ("0x00", "0x7F"):
        env = dict(os.environ, BSLV_FILL=fill, BSLV_CASES="covering-40x20x4")
        env.pop("BSLV_ALLOC_LOG", None)
        rows.append(_spawn(["fill", vfile], env, timeout=300))
    assert rows[0] == rows[1]
    assert rows[0]["w"] == out[1]["w"].tobytes().hex()


if __name__ == "__main__":
    from bensolve_amd import synth
    what, V = sys.argv[1], np.load(sys.argv[2])
    if what == "helpers":
        model = _wide_model(2049)
    else:
        name = os.environ["BSLV_CASES"]
        model = P2Model(cc.octahedron_vlp() if name == "octahedron" else synth.covering_vlp(40, 20, 4, 9))
    print(json.dumps(_child_batch(model, V)))
