"""GPU: the LP engine under its default method (DUAL) on general models -- all five bound types, negative coefficients, equality
and ranged rows, free and boxed columns, a cost shift -- in batches that mix OPTIMAL and INFEASIBLE LPs, at the shapes where the launch
code of bensolve_amd/csrc/lp_engine.hip changes its mind.  The LPs, the two CPU yardsticks (the oracle's primal simplex and HiGHS) and
the certificate are tests/lp_cases.py's; `python tests/lp_cases.py` shows without a GPU that the yardsticks agree on every LP.

Shapes (M, N) and the threshold each pair straddles (lines of lp_engine.hip):
  (15, 16) (16, 17)      ld = ceil16(N): 16 against 32 (raw_create, "L.ld = (N + 15) / 16 * 16"); Mp1p = ceil16(M + 1): 16 against 32
                         ("L.Mp1p = (M + 1 + 15) / 16 * 16"); M + 1 = 16, 17 against k_flush's rows per tile tr = 4 .. 32 (solve_batch_impl,
                         "int tr = running * tiles >= 2048 ? 32 : ...": 4 for one LP, 4 or 8 for 16)
  (31, 64) (32, 65)      one wave of 64 columns against two; ld = 64 against 80; Mp1p = 32 against 48; M + 1 = 32 against 33: the last
                         tile of tr rows full against one row
  (33, 257)              one workgroup of NT = 256 columns against two; M + 1 = 34: no multiple of any tr
  (24, 1120) (24, 1121)  the 1024-thread k_flush: "big_flush = ... lds > 53 * 1024" with lds = KP * ldt * 8, ldt = 1120 against 1136
                         (tr = 16 .. 128 there; M + 1 = 25)
  (24, 1535) (24, 1536)  the selection with NT_BIG threads: plan_select, "L.N >= 1536 ? NT_BIG : NT"
  (24, 2048) (24, 2049)  the 2048 columns of k_init_grouped (plan_init; wider rows start with k_init) and, in the revised form, one
                         slice of REV_SLICE = 2048 columns against two ("rev_nslices")
  (24, 4100)             revised form only: three slices, so that helper workgroups take some (rev_helper / rev_take_slices)
KP = 6 pending pivots and REFRESH_AFTER = 32 are thresholds in the number of pivots of a solve: the last test asserts that the sets
hold OPTIMAL LPs with 1 .. 6, with 7 .. 12 and with more than 32 pivots.

Per shape one model and 16 LPs that differ in the bounds of the per-LP range, in two arrangements (lp_cases.general_set): "a" every
row per LP, "b" up to 40 columns from column 1 per LP (min(N, 40) columns do not fit behind an odd start where N <= 40: N - 2 there,
the last column is the one with the artificial bound and keeps the model's bounds).
LP 5 is infeasible by construction.  A run: LP 0 cold into slot 0; all 16 from slot 0 in one batch; each alone and the first 7
together from slot 0; a second generation from the slots of the first with the bounds permuted, together and alone; the second
generation again in place.

Run as a program (`python tests/test_lp_general_gpu.py child`) it runs the (24, 4100) set of arrangement "a" in the form the
environment asks for and prints a SHA-256 of everything it got: the helper-count test starts it that way."""
import contextlib
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bensolve_amd.lp import LpEngine
import lp_cases as lc
from lp_cases import RTOL, OPTIMAL, INFEASIBLE, UNBOUNDED, UNDEFINED, NLP, BAD

pytestmark = pytest.mark.gpu

SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 1120), (24, 1121), (24, 1535), (24, 1536), (24, 2048), (24, 2049)]
REV_SHAPES = [(33, 257), (24, 1536), (24, 2049), (24, 4100)]          # 1, 1, 2 and 3 slices
EXT_SHAPES = [(32, 65), (24, 1536)]
NONE = np.zeros((1, 0))
# slots: 0 the parent; the batch; its LPs alone; the second generation; scratch (the sub-batch of 7, then the second generation alone)
GEN1, ALONE, GEN2, SCRATCH = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(4))
POOL = 1 + 4 * NLP
SUB = 7


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(A, lo, up, cost, first, cnt, slots, form):
    """form: "tableau" (BSLV_LP_REV unset: what create chooses by itself at these sizes), "revised" (BSLV_LP_REV=1, read at create) or
    "extended" (the tableau form with set_extended(1))"""
    M, N = A.shape
    with _env(BSLV_LP_REV="1" if form == "revised" else None):
        eng = LpEngine(M, N, A, lo, up, cost, first, cnt, slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [__import__("ctypes").c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(form == "revised")
    if form == "extended":
        eng.set_extended(1)
    return eng


def _solve(eng, src, dst, vlo, vup, retry):
    """one batch; retry (the revised form): an LP that comes back UNDEFINED is solved once more from a reset slot, as the header tells
    callers to.  Returns statuses, pivots and the number of retries."""
    st, it = eng.solve_batch(src, dst, vlo, vup)
    st, it, n = st.copy(), it.copy(), 0
    if retry:
        for b in np.nonzero(st == UNDEFINED)[0]:
            eng.reset_slot(int(dst[b]))
            s1, i1 = eng.solve_batch([dst[b]], [dst[b]], vlo[b:b + 1], vup[b:b + 1])
            st[b], it[b], n = s1[0], it[b] + i1[0], n + 1
    return st, it, n


def _read(eng, dst, st, it):
    n = eng.M + eng.N
    return dict(st=np.array(st), it=np.array(it), obj=eng.obj(dst), prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n))


_RUNS = {}


def _run(M, N, arr, form):
    """every solve of one set in one form, once: the tests only look at the record"""
    key = (M, N, arr, form)
    if key in _RUNS:
        return _RUNS[key]
    s = lc.general_set(M, N, arr)
    vlo, vup, perm = s["vlo"], s["vup"], s["perm"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, form)
    rec = dict(retries=0)
    eng.reset_slot(0)
    st, it, n = _solve(eng, [0], [0], vlo[:1], vup[:1], retry)
    rec["cold"] = _read(eng, [0], st, it)
    rec["retries"] += n
    zeros = np.zeros(NLP, np.int32)
    st, it, n = _solve(eng, zeros, GEN1, vlo, vup, retry)
    rec["gen1"] = _read(eng, GEN1, st, it)
    rec["retries"] += n
    if form == "tableau":
        st, it = [], []
        for b in range(NLP):
            s1, i1 = eng.solve_batch([0], [ALONE[b]], vlo[b:b + 1], vup[b:b + 1])
            st.append(s1[0]); it.append(i1[0])
        rec["gen1_alone"] = _read(eng, ALONE, st, it)
        st, it = eng.solve_batch(zeros[:SUB], SCRATCH[:SUB], vlo[:SUB], vup[:SUB])
        rec["gen1_sub"] = _read(eng, SCRATCH[:SUB], st, it)
    st, it, n = _solve(eng, GEN1, GEN2, vlo[perm], vup[perm], retry)
    rec["gen2"] = _read(eng, GEN2, st, it)
    rec["retries"] += n
    if form == "tableau":
        st, it = [], []
        for b in range(NLP):
            s1, i1 = eng.solve_batch([GEN1[b]], [SCRATCH[b]], vlo[perm[b]][None], vup[perm[b]][None])
            st.append(s1[0]); it.append(i1[0])
        rec["gen2_alone"] = _read(eng, SCRATCH, st, it)
    st, it = eng.solve_batch(GEN2, GEN2, vlo[perm], vup[perm])
    rec["again"] = _read(eng, GEN2, st, it)
    eng.close()
    _RUNS[key] = rec
    return rec


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_identical(a, b, tag, sel=slice(None)):
    for k in ("st", "obj", "prim", "dual"):
        assert _same_bits(a[k][sel], b[k]), (tag, k, a["it"][sel], b["it"])


def _assert_against_references(s, ref, oracle_gap, got, lps, form, tag):
    """statuses, objectives (both yardsticks) and the certificate of every OPTIMAL LP of one batch; returns the certificates"""
    certs = []
    for b, t in enumerate(lps):
        r = ref[t]
        assert got["st"][b] == r["st"], (tag, b, t, got["st"], [ref[u]["st"] for u in lps])
        if r["st"] != OPTIMAL:
            continue
        np.testing.assert_allclose(got["obj"][b], r["obj"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d" % (tag, t))
        np.testing.assert_allclose(got["obj"][b], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d (HiGHS)" % (tag, t))
        lo, up = s["lps"][t]
        c = lc.certify(s["A"], lo, up, s["cost"], int(got["st"][b]), got["obj"][b], got["prim"][b], got["dual"][b])
        certs.append(c)
        lc.assert_certified(c, got["obj"][b], oracle_gap, (tag, b, t))
    return certs


def _report(form, M, N, arr, certs, oracle):
    w = lc.worst(certs)
    print("lp_general_residuals engine %s M %d N %d arr %s lps %d rows %.3e feas %.3e dj %.3e side %.3e gap %.3e (oracle gap %.3e)" % (
        form, M, N, arr, len(certs), w["rows"], w["feas"], w["dj"], w["side"], w["gap"], oracle["gap"]))


def _check_run(M, N, arr, form):
    s = lc.general_set(M, N, arr)
    ref, oracle = lc.assert_references_agree(M, N, arr)          # (the yardsticks agree: checked when the seeds were chosen)
    rec = _run(M, N, arr, form)
    perm = s["perm"]
    tag = (form, M, N, arr)
    print("pivots %s: cold %s gen1 %s gen2 %s retries %d" % (tag, rec["cold"]["it"], rec["gen1"]["it"], rec["gen2"]["it"], rec["retries"]))
    certs = _assert_against_references(s, ref, oracle["gap"], rec["cold"], [0], form, tag + ("cold",))
    certs += _assert_against_references(s, ref, oracle["gap"], rec["gen1"], range(NLP), form, tag + ("gen1",))
    certs += _assert_against_references(s, ref, oracle["gap"], rec["gen2"], perm, form, tag + ("gen2",))
    _report(form, M, N, arr, certs, oracle)
    assert not np.any(rec["gen1"]["st"] == UNDEFINED) and not np.any(rec["gen2"]["st"] == UNDEFINED)
    # again in place: nothing to do for an LP that is solved, and the same answer
    again, gen2 = rec["again"], rec["gen2"]
    assert np.array_equal(again["st"], gen2["st"]), (tag, again["st"], gen2["st"])
    opt = gen2["st"] == OPTIMAL
    assert np.all(again["it"][opt] == 0), (tag, again["it"])
    np.testing.assert_allclose(again["obj"][opt], gen2["obj"][opt], rtol=RTOL, atol=1e-9)
    for k in ("prim", "dual"):          # (beta is recomputed from the tableau at the start of a solve: 1e-8, the project's figure for a value against its bound)
        np.testing.assert_allclose(again[k][opt], gen2[k][opt], rtol=RTOL, atol=1e-8, err_msg=str(tag + (k,)))
    return rec


# ---- 1. the default method, tableau form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_default_method_on_a_general_set(oracle, M, N, arr):
    rec = _check_run(M, N, arr, "tableau")
    assert rec["retries"] == 0
    # a mixed batch is its LPs alone, bit for bit: the batch of 16, its first 7, the second generation
    assert rec["gen1"]["st"][BAD] == INFEASIBLE and np.sum(rec["gen1"]["st"] == OPTIMAL) >= 12
    _assert_identical(rec["gen1"], rec["gen1_alone"], (M, N, arr, "16 against 1"))
    _assert_identical(rec["gen1"], rec["gen1_sub"], (M, N, arr, "16 against 7"), sel=slice(0, SUB))
    _assert_identical(rec["gen2"], rec["gen2_alone"], (M, N, arr, "second generation, 16 against 1"))


@pytest.mark.parametrize("M,N,form", [(M, N, "tableau") for M, N in SHAPES] + [(M, N, "revised") for M, N in REV_SHAPES])
def test_unbounded_model(oracle, M, N, form):
    """a free column with a cost and no row: the artificial bound the DUAL start gives it is where the LP ends, and the answer is UNBOUNDED"""
    A, lo, up, cost = lc.unbounded_model(M, N)
    assert lc.oracle_primal(A, lo, up, cost)[0] == UNBOUNDED and lc.highs(A, lo, up, cost)[0] == UNBOUNDED
    eng = _engine(A, lo, up, cost, 0, 0, 2, form)
    eng.reset_slot(0)
    st, it, _ = _solve(eng, [0], [0], NONE, NONE, form == "revised")
    eng.close()
    assert st[0] == UNBOUNDED, (M, N, form, st, it)


# ---- 2. the same LPs in the revised form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", REV_SHAPES)
def test_revised_form_on_a_general_set(oracle, M, N, arr):
    rec = _check_run(M, N, arr, "revised")           # (statuses against the references, none UNDEFINED after one retry)
    tab = _run(M, N, arr, "tableau")
    for gen in ("cold", "gen1", "gen2"):
        assert np.array_equal(rec[gen]["st"], tab[gen]["st"]), (M, N, arr, gen, rec[gen]["st"], tab[gen]["st"])
        opt = tab[gen]["st"] == OPTIMAL
        np.testing.assert_allclose(rec[gen]["obj"][opt], tab[gen]["obj"][opt], rtol=RTOL, atol=1e-9)


def _digest(rec):
    h = hashlib.sha256()
    for gen in ("cold", "gen1", "gen2", "again"):
        for k in ("st", "it", "obj", "prim", "dual"):
            h.update(np.ascontiguousarray(rec[gen][k]).tobytes())
    return h.hexdigest()


def _child():
    form = "revised" if os.environ.get("BSLV_LP_REV") == "1" else "tableau"
    rec = _run(24, 4100, "a", form)
    print("helpers %s statuses %s retries %d" % (os.environ.get("BSLV_REV_HELPERS"), "".join(str(v) for v in rec["gen1"]["st"]), rec["retries"]))
    print("sha256 " + _digest(rec))


def test_revised_form_does_not_depend_on_the_number_of_helpers(oracle):
    """BSLV_REV_HELPERS (read once per process) caps the workgroups that share the slices of a tableau row: 1 = the LP's own workgroup
    takes all three slices of the (24, 4100) set, 2, and unset = one workgroup per slice.  Who took a slice must not show in any bit."""
    ref, _ = lc.assert_references_agree(24, 4100, "a")
    out = []
    for helpers in ("1", "2", None):
        env = dict(os.environ, BSLV_LP_REV="1")
        env.pop("BSLV_REV_HELPERS", None)
        if helpers:
            env["BSLV_REV_HELPERS"] = helpers
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, "helpers %s: rc %d\n%s" % (helpers, p.returncode, p.stderr[-1500:])      # (the first child that fails ends the test)
        lines = p.stdout.strip().splitlines()
        print(lines[-2])
        assert lines[-2].split()[3] == "".join(str(r["st"]) for r in ref), lines[-2]
        out.append(lines[-1])
    assert out[0].startswith("sha256 ") and out[0] == out[1] == out[2], out


# ---- 3. the extended selection --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", EXT_SHAPES)
def test_extended_selection_on_a_general_set(oracle, M, N, arr):
    """bound flipping, perturbation and the primal clean-up on sets with boxed variables"""
    rec = _check_run(M, N, arr, "extended")
    assert rec["retries"] == 0
    tab = _run(M, N, arr, "tableau")
    for gen in ("cold", "gen1", "gen2"):
        assert np.array_equal(rec[gen]["st"], tab[gen]["st"]), (M, N, arr, gen)
        opt = tab[gen]["st"] == OPTIMAL
        np.testing.assert_allclose(rec[gen]["obj"][opt], tab[gen]["obj"][opt], rtol=RTOL, atol=1e-9)


# ---- 4. the sets reach the thresholds in the number of pivots ----------------------------------------------------------------
def test_pivot_counts_cover_the_bands(oracle):
    """KP = 6: a solve of 1 .. 6 pivots has one pass over its tableau, one of 7 .. 12 two; REFRESH_AFTER = 32: beyond it optimality is
    only declared on a recomputed beta.  Over the shapes together some OPTIMAL LP has to fall into each of the three bands."""
    counts = []
    for M, N in SHAPES:
        for arr in ("a", "b"):
            rec = _run(M, N, arr, "tableau")
            for gen in ("cold", "gen1", "gen2"):
                counts += [int(i) for i, st in zip(rec[gen]["it"], rec[gen]["st"]) if st == OPTIMAL]
    counts = np.array(counts)
    edges = [0, 1, 7, 13, 33, 1 << 30]
    hist = [int(np.sum((counts >= a) & (counts < b))) for a, b in zip(edges[:-1], edges[1:])]
    print("pivots of the OPTIMAL LPs: 0: %d, 1..6: %d, 7..12: %d, 13..32: %d, more than 32: %d (max %d)" % (*hist, counts.max()))
    assert hist[1] > 0 and hist[2] > 0 and hist[4] > 0, hist


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "child":
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        _child()
