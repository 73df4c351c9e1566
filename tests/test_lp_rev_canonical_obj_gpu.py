"""GPU: canonical optimal points of objective batches PER CALL (bslv_lpq_solve_batch_obj_canonical), in the revised form above all --
its tie phase is k_select_tie_obj_rev / tie_obj_once<true> of bensolve_amd/csrc/lp_engine.hip, and this call is the only way to it.

The protocol is tests/test_lp_canonical_obj_gpu.py's (_start / _batch): the feasibility LP in slot 0, PART 1's in-place objective solve
there, then ONE batch of all kept weights from slot 0 -- once by solve_batch_obj and once by the new call, each on an engine of its
own.  Expected canonical points are canonical_obj_cases' (HiGHS on the shifted weights, nothing from the code under test), for its five
sets and the two wide ones of canonical_obj_rev_cases (N = 2048 and N = 2049: the first shape with a helper workgroup); the bound is
that test's, RTOL = ATOL = 1e-9.  The revised form is forced with BSLV_LP_REV=1 at create and asserted with bslv_lpq_is_revised.

Run as a script it is the child of three tests (the environment is read once per process): `helpers W.npy`, `drift W.npy` and
`fill W.npy` each print one JSON line."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import canonical_cases as cc
import canonical_obj_cases as co
import canonical_obj_rev_cases as cr
from bensolve_amd._lib import BslvError
from test_lp_canonical_obj_gpu import _batch, _check_certificates, _start
from test_lp_general_gpu import _env, _same_bits

pytestmark = pytest.mark.gpu
OPTIMAL = 4
E_ARG = 2
RTOL = ATOL = 1e-9        # tests/test_lp_canonical_obj_gpu.py's bound against HiGHS
ZERO = dict(entered=0, tie_iters=0, unbounded=0, capped=0)
WIDE_HELPER = cr.WIDE[2049]
# LpEngine.certify's six tolerances (rows, feas, dj, side, gap x (1 + |z|), dual zero) set to what _check_certificates of
# tests/test_lp_canonical_obj_gpu.py applies: y = P x and A x >= 1 at 1e-8, a dual's sign at 1e-9, "at a bound" at 1e-8, the objective
# from the duals at 1e-8, a dual counts as zero up to 1e-9 (its `small` window)
CERT_TOL = (1e-8, 1e-8, 1e-9, 1e-8, 1e-8, 1e-9)


def _start_form(model, slots, form="revised"):
    with _env(BSLV_LP_REV="1" if form == "revised" else None):
        eng = _start(model, slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(form == "revised")
    return eng


def _batch_call(eng, model, W, src=None, dst=None, ddir="default", first=None):
    B = len(W)
    src = np.zeros(B, np.int32) if src is None else np.asarray(src, np.int32)
    dst = np.arange(1, B + 1, dtype=np.int32) if dst is None else np.asarray(dst, np.int32)
    st, it = eng.solve_batch_obj_canonical(cc.direction(model.q) if isinstance(ddir, str) else ddir, src, dst, model.y_first if first is None else first, W)
    return dst, st, it


def _read(eng, model, dst, st, it):
    n = model.M + model.N
    return dict(st=st.copy(), it=it.copy(), obj=eng.obj(dst), y=eng.primal(dst, model.y_first, model.q), val=eng.primal(dst, 0, n),
                dual=eng.dual(dst, 0, n), stats=eng.last_canonical_obj_stats(),
                last={k: v for k, v in eng.last_stats().items() if not k.endswith("_ms")})


_runs = {}


def _run(name):
    """a case set on revised engines, once: by solve_batch_obj (0) and by the new call (1)"""
    if name not in _runs:
        prob, c = cr.cases(name)
        if name in cr.COVERING:
            co.check_case_set(c)
        model = co.P1Model(prob)
        out = {}
        for on in (0, 1):
            eng = _start_form(model, len(c["W"]) + 1)
            dst, st, it = (_batch_call if on else _batch)(eng, model, c["W"])
            out[on] = _read(eng, model, dst, st, it)
            out[on]["get"] = eng.get_canonical_obj()
            eng.close()
        _runs[name] = (prob, c, model, out)
    return _runs[name]


def _off_differs(c, off):
    return np.abs(off["y"] - c["y"]).max(axis=1) > 1e-6


# ---- 1. expected points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.ALL)
def test_the_call_ends_in_the_expected_point(name):
    prob, c, model, out = _run(name)
    off, on = out[0], out[1]
    assert np.all(off["st"] == OPTIMAL) and np.all(on["st"] == OPTIMAL), (off["st"], on["st"])
    print("lp_rev_canonical_obj %s (%d x %d): %d cases, %d degenerate; y of solve_batch_obj differs from the canonical y by more than 1e-6 in %d; tie phase %s"
          % (name, model.M, model.N, len(c["W"]), int(c["degenerate"].sum()), int(_off_differs(c, off).sum()), on["stats"]))
    print("   largest |y_on - y_expected| / (1 + |y|): %.3e" % (np.abs(on["y"] - c["y"]) / (1.0 + np.abs(c["y"]))).max())
    np.testing.assert_allclose(on["obj"], off["obj"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(off["obj"], c["z"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(on["obj"], c["z"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(on["y"], c["y"], rtol=RTOL, atol=ATOL)
    assert on["get"] == 0 and off["get"] == 0
    if name in cr.DECOYS:
        V = co.decoy_vertices(model.q)
        for y in on["y"]:
            assert np.abs(V - y).max(axis=1).min() <= 1e-9, y


# ---- 2. counters ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.ALL)
def test_counters(name):
    prob, c, model, out = _run(name)
    off, on = out[0], out[1]
    s = on["stats"]
    assert 0 < s["entered"] <= len(c["W"])
    assert s["tie_iters"] >= int((c["degenerate"] & _off_differs(c, off)).sum())
    assert s["capped"] == 0 and s["unbounded"] == 0
    assert int(on["it"].sum()) - int(off["it"].sum()) == s["tie_iters"]      # tie iterations are counted in iters[]
    assert off["stats"] == ZERO                                              # after a plain solve_batch_obj


# ---- 3. the start does not matter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.ALL)
def test_the_start_does_not_matter(name):
    """case k from the canonical slot of case k - 1; then in place on those slots: no iteration, no tie iteration, the same y"""
    prob, c, model, out = _run(name)
    W = c["W"]
    B = len(W)
    eng = _start_form(model, 2 * B + 1)
    try:
        dst, st, _ = _batch_call(eng, model, W)
        assert np.all(st == OPTIMAL)
        dst2 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
        _, st, _ = _batch_call(eng, model, W, src=np.roll(dst, 1), dst=dst2)
        assert np.all(st == OPTIMAL)
        y2 = eng.primal(dst2, model.y_first, model.q)
        print("lp_rev_canonical_obj %s: largest |y - expected| from a sibling's slot: %.3e" % (name, np.abs(y2 - c["y"]).max()))
        np.testing.assert_allclose(y2, c["y"], rtol=RTOL, atol=ATOL)
        _, st, it = _batch_call(eng, model, W, src=dst2, dst=dst2)
        assert np.all(st == OPTIMAL)
        assert np.all(it == 0), it
        assert eng.last_canonical_obj_stats()["tie_iters"] == 0
        np.testing.assert_allclose(eng.primal(dst2, model.y_first, model.q), c["y"], rtol=RTOL, atol=ATOL)
    finally:
        eng.close()


# ---- children -------------------------------------------------------------------------------------------------------------------------------
def _child_record(name, W):
    """the new call on a revised engine, as one JSON-able record of bits"""
    prob = cr.VLP[name]()
    model = co.P1Model(prob)
    eng = _start_form(model, len(W) + 1)
    dst, st, it = _batch_call(eng, model, W)
    r = _read(eng, model, dst, st, it)
    eng.close()
    return dict(st=r["st"].tolist(), it=r["it"].tolist(), obj=r["obj"].tobytes().hex(), y=r["y"].tobytes().hex(),
                sha=hashlib.sha256(np.ascontiguousarray(r["y"]).tobytes()).hexdigest(), stats=r["stats"])


def _spawn(args, env, timeout=240):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert "Memory access fault" not in p.stderr, "%s: %s" % (args, p.stderr[-800:])
    assert p.returncode == 0, "%s: rc %d\n%s" % (args, p.returncode, p.stderr[-1500:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def _child_env(**kv):
    env = {k: v for k, v in os.environ.items() if k not in ("BSLV_REV_HELPERS", "BSLV_LP_REV_DRIFT", "BSLV_FILL", "BSLV_ALLOC_LOG")}
    env.update(kv)
    return env


# ---- 4. helpers do not change a bit -----------------------------------------------------------------------------------------------------------
def test_helpers_do_not_change_a_bit(tmp_path):
    """N = 2049 with one workgroup per LP (BSLV_REV_HELPERS=1) and with the default, a helper beside it: y, objective and iteration
    counts are the same bits.  The variable is read once per process: a child each (the first that fails ends the test)"""
    prob, c, model, out = _run(WIDE_HELPER)
    wfile = str(tmp_path / "W.npy")
    np.save(wfile, c["W"])
    rows = [_spawn(["helpers", WIDE_HELPER, wfile], _child_env(**({"BSLV_REV_HELPERS": h} if h else {}))) for h in ("1", None)]
    assert rows[0] == rows[1]
    assert rows[1]["stats"]["tie_iters"] > 0
    assert rows[1]["y"] == out[1]["y"].tobytes().hex() and rows[1]["it"] == out[1]["it"].tolist()


# ---- 5. tableau form: the call IS set_canonical_obj(1, ..); solve_batch_obj; the old switch back ----------------------------------------------
@pytest.mark.parametrize("name", ["decoy-3", "covering-30x80x3"])
@pytest.mark.parametrize("switch", ["off", "other"])
def test_tableau_form_the_call_is_the_switch_for_one_batch(name, switch):
    """twin engines in the tableau form, once with the engine's switch off and once with it on for ANOTHER direction -- which
    get_canonical_obj and a following plain solve_batch_obj must still show, as on an engine that never saw the call"""
    prob, c = cr.cases(name)
    model = co.P1Model(prob)
    W, B = c["W"], len(c["W"])
    d = cc.direction(model.q)
    other = d[::-1].copy() * np.array([1.0 + 0.25 * j for j in range(len(d))])
    rows = []
    for by_call in (True, False):
        eng = _start_form(model, 2 * B + 1, "tableau")
        if switch == "other":
            assert eng.set_canonical_obj(1, model.y_first, other) == 0
        if by_call:
            dst, st, it = _batch_call(eng, model, W, ddir=d)
        else:
            assert eng.set_canonical_obj(1, model.y_first, d) == 0
            dst, st, it = _batch(eng, model, W)
            assert (eng.set_canonical_obj(1, model.y_first, other) if switch == "other" else eng.set_canonical_obj(0)) == 0
        assert eng.get_canonical_obj() == int(switch == "other")
        rec = _read(eng, model, dst, st, it)
        dst2, st2, it2 = _batch(eng, model, W, dst=np.arange(B + 1, 2 * B + 1, dtype=np.int32))
        rec.update({"next_" + k: v for k, v in _read(eng, model, dst2, st2, it2).items()})
        eng.close()
        rows.append(rec)
    a, b = rows
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert _same_bits(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    np.testing.assert_allclose(a["y"], c["y"], rtol=RTOL, atol=ATOL)
    assert a["stats"]["tie_iters"] > 0
    if switch == "off":
        assert a["next_stats"] == ZERO
    else:
        assert a["next_stats"]["entered"] == B      # (the engine's own switch and direction are in force again)


# ---- 6. bad arguments -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["revised", "tableau"])
def test_bad_arguments_change_nothing(form):
    """a NaN or an inf in ddir, ddir = NULL, a bad range: BSLV_E_ARG, and the next batch is the same bits as on an engine that never
    saw the bad calls; the engine-wide switch of the revised form keeps its refusal"""
    prob, c = cr.cases("decoy-3")
    model = co.P1Model(prob)
    W, B = c["W"], len(c["W"])
    d = cc.direction(model.q)
    rows = []
    for bad in (True, False):
        eng = _start_form(model, B + 1, form)
        if bad:
            nan, inf = d.copy(), d.copy()
            nan[1], inf[-1] = np.nan, np.inf
            for dd, first in ((nan, None), (inf, None), (None, None), (d, -1), (d, model.M + model.N - 1)):
                with pytest.raises(BslvError, match="error 2"):
                    _batch_call(eng, model, W, ddir=dd, first=first)
                assert "bslv_lpq_solve_batch_obj_canonical" in eng.lib.bslv_last_error().decode()
            assert eng.get_canonical_obj() == 0
        if form == "revised":
            assert eng.set_canonical_obj(1, model.y_first, d) == E_ARG and "revised" in eng.lib.bslv_last_error().decode()
            assert eng.get_canonical_obj() == 0
        dst, st, it = _batch(eng, model, W)
        rows.append(_read(eng, model, dst, st, it))
        eng.close()
    for k in ("st", "it", "obj", "val", "dual"):
        assert _same_bits(rows[0][k], rows[1][k]), k
    assert rows[0]["last"] == rows[1]["last"] and rows[0]["stats"] == rows[1]["stats"] == ZERO


# ---- 7. the drift hook reaches a tie pivot ------------------------------------------------------------------------------------------------------
def test_a_tie_pivot_that_fails_the_cross_check_keeps_the_optimum(tmp_path):
    """decoy-3 (no column has a finite upper bound: every tie iteration is a pivot) under BSLV_LP_REV_DRIFT=b:p with p = the plain
    solve's iters[b] + 1, the first tie pivot of LP b.  Nothing is committed: LP b stays OPTIMAL with the plain solve's bits in
    objective, y and iters and counts in stats[3]; every other LP is as without the hook"""
    name = "decoy-3"
    prob, c, model, out = _run(name)
    off, on = out[0], out[1]
    tied = np.nonzero(on["it"] > off["it"])[0]
    tied = tied[tied > 0]          # (the hook names an LP by its index in a batch, and the solves of the start are LP 0 of their own)
    assert len(tied) > 0
    b = int(tied[0])
    wfile = str(tmp_path / "W.npy")
    np.save(wfile, c["W"])
    row = _spawn(["drift", name, wfile], _child_env(BSLV_LP_REV_DRIFT="%d:%d" % (b, int(off["it"][b]) + 1)))
    st, it = np.array(row["st"]), np.array(row["it"])
    y = np.frombuffer(bytes.fromhex(row["y"])).reshape(-1, model.q)
    obj = np.frombuffer(bytes.fromhex(row["obj"]))
    print("lp_rev_canonical_obj drift: LP %d at pivot %d; tie phase %s" % (b, int(off["it"][b]) + 1, row["stats"]))
    assert st[b] == OPTIMAL and obj[b].tobytes() == off["obj"][b].tobytes()
    assert it[b] == off["it"][b] and y[b].tobytes() == off["y"][b].tobytes()      # (the basis the plain solve ends in)
    assert row["stats"]["capped"] == 1
    others = np.arange(len(st)) != b
    assert np.array_equal(st[others], on["st"][others]) and np.array_equal(it[others], on["it"][others])
    assert y[others].tobytes() == on["y"][others].tobytes() and obj[others].tobytes() == on["obj"][others].tobytes()


# ---- 8. fill byte ---------------------------------------------------------------------------------------------------------------------------
def test_the_call_does_not_depend_on_the_fill_byte(tmp_path):
    """fresh device memory filled with 0x00 and with 0x7F, a child each: the same y, bit for bit (the phase reads nothing it has not
    written)"""
    name = "covering-30x80x3"
    prob, c, model, out = _run(name)
    wfile = str(tmp_path / "W.npy")
    np.save(wfile, c["W"])
    rows = [_spawn(["fill", name, wfile], _child_env(BSLV_FILL=fill), timeout=300) for fill in ("0x00", "0x7F")]
    print([r["sha"] for r in rows], rows[0]["stats"])
    assert rows[0]["sha"] == rows[1]["sha"] and rows[0] == rows[1]
    assert rows[0]["stats"]["tie_iters"] > 0
    assert rows[0]["y"] == out[1]["y"].tobytes().hex()


# ---- 9. certificate ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["covering-40x20x4", "decoy-4"])
def test_certificates(name):
    """the device's own certificate of the destination slots after the call (LpEngine.certify, at the bounds of
    test_lp_canonical_obj_gpu._check_certificates), and that check itself on the values read back"""
    prob, c = cr.cases(name)
    model = co.P1Model(prob)
    W = c["W"]
    eng = _start_form(model, len(W) + 1)
    try:
        dst, st, it = _batch_call(eng, model, W)
        assert np.all(st == OPTIMAL)
        cert = eng.certify(dst, cost_first=model.y_first, costs=W, tol=CERT_TOL)
        print("lp_rev_canonical_obj %s: largest residuals (rows, feas, dj, side, gap) %s" % (name, cert["res"].max(axis=0)))
        assert np.all(cert["verdict"] == 0), (cert["verdict"], cert["res"], cert["at"])
        assert eng.last_certify_stats()["not_certified"] == 0
        r = _read(eng, model, dst, st, it)
        _check_certificates(model, prob, r["val"], r["dual"], W, r["obj"])
    finally:
        eng.close()


if __name__ == "__main__":
    what, name, W = sys.argv[1], sys.argv[2], np.load(sys.argv[3])
    assert what in ("helpers", "drift", "fill")
    print(json.dumps(_child_record(name, W)))
