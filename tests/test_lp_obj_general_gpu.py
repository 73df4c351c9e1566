"""GPU: batches of LPs that differ in their objective (bslv_lpq_solve_batch_obj) on general models -- all five bound types on rows and
columns, boxed and fixed columns, ranged and equality rows, cost on nonbasic bounded variables and on row variables -- in both forms of
the LP engine, at the shapes where the launch code of bensolve_amd/csrc/lp_engine.hip changes its mind.  The models, the cost vectors,
the two CPU yardsticks (the oracle's primal simplex and HiGHS, on the cost folded onto the columns) and the certificate are
tests/lp_cases.py's; `python tests/lp_cases.py obj` shows without a GPU that the yardsticks agree on every LP.

Shapes (M, N) and the threshold each pair straddles (lines of lp_engine.hip):
  (15, 16) (16, 17)      ld = ceil16(N): 16 against 32 (raw_create, "L.ld = (N + 15) / 16 * 16"); Mp1p = ceil16(M + 1): 16 against 32
                         ("L.Mp1p = (M + 1 + 15) / 16 * 16"); k_flush's rows per tile (solve_batch_impl, "int tr = running * tiles >= 2048 ? 32 : ...")
  (31, 64) (32, 65)      one wave of 64 columns against two; ld = 64 against 80; Mp1p = 32 against 48; plan_select's "while (cap2 < L.N)
                         cap2 <<= 1": 64 against 128
  (33, 257)              one workgroup of NT = 256 columns against two (k_prep's "for (int j = threadIdx.x; j < L.ld; j += NT)", whose
                         objmode branch builds the new reduced-cost row)
  (24, 512) (24, 513)    revised form: one slice of REV_PRICE_SLICE = 2 * NT = 512 columns of k_rev_price against two ("dim3((L.ld +
                         REV_PRICE_SLICE - 1) / REV_PRICE_SLICE, B)")
  (24, 1024) (24, 1025)  cap2 = 1024 against 2048
  (24, 1120) (24, 1121)  the 1024-thread k_flush: "big_flush = ... lds > 53 * 1024" with lds = KP * ldt * 8, ldt = 1120 against 1136
  (24, 1535) (24, 1536)  the selection with NT_BIG threads: plan_select, "L.N >= 1536 ? NT_BIG : NT"
  (24, 2048) (24, 2049)  cap2 = 2048 against 4096; in the revised form one slice of REV_SLICE = 2048 columns against two ("rev_nslices")
  (24, 4100)             revised form only: three slices, helper workgroups take some
  (24, 8192) (24, 8193)  plan_select, "if (bfrt && sel_lds > 144 * 1024) { cap2 = 0; ...": sel_lds = 12 * cap2 + N is 106 496 bytes at
                         N = 8192 and, with cap2 = 16384, over the limit at 8193: the extended selection without its long-step part
An objective batch never starts with k_init_grouped (plan_init, "!on || L.objmode"), always runs k_select<true> (plan_select, "bfrt =
h->has_boxed || L.objmode || ...") and takes primal steps (k_prep, "Bv.pflags[b] = (L.objmode || ...) ? PF_PRIMAL : 0").

Cost ranges (lp_cases.cost_range): "cols" every column (cost_cnt = N: the loop "for (int t = 0; t < L.ccnt; t++)" of k_prep and
k_rev_price over pos[cfirst + t], and a cost on every nonbasic column, "if (kj >= 0 && kj < L.ccnt) v = cv[kj]"); "straddle" three
row variables and five columns; "head" five columns from the odd start M + 1.

A run (one per shape, range and form, recorded once, the tests read the record): the feasibility LP into slot 0 (solve_batch, zero
cost); generation 1, 16 LPs from slot 0 in one batch; each of them alone and the first 7 together; generation 2 from the slots of
generation 1, together and alone; generation 3 in place on the slots of generation 2, and once more; a mixed batch with the costs of
generation 2, the even LPs from slot 0 and the odd ones from their slots of generation 1.

Run as a program (`python tests/test_lp_obj_general_gpu.py child`) it runs the (24, 1025) "cols" set in the tableau form and prints a
SHA-256 of everything it read: the fill-byte test starts it that way."""
import hashlib
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

import lp_cases as lc
from lp_cases import RTOL, OPTIMAL, UNBOUNDED, UNDEFINED, NLP, GENS
from test_lp_general_gpu import _env, _engine, _read, _assert_identical

pytestmark = pytest.mark.gpu

SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 1024), (24, 1025), (24, 1120), (24, 1121), (24, 1535), (24, 1536),
          (24, 2048), (24, 2049), (24, 8192), (24, 8193)]
REV_SHAPES = [(33, 257), (24, 512), (24, 513), (24, 1536), (24, 2049), (24, 4100)]
SIDE_SHAPES = [(32, 65), (24, 1536)]            # the per-LP bound range and the unbounded objectives
NONE = np.zeros((1, 0))
# slots: 0 the parent; generation 1; its LPs alone; generations 2 and 3; scratch (the sub-batch of 7, then generation 2 alone); the mixed batch
GEN1, ALONE, GEN2, SCRATCH, MIX = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(5))
POOL = 1 + 5 * NLP
SUB = 7
BATCHES = ("gen1", "gen2", "gen3", "mix")       # the batches of a record that are checked against the references ...
REF_GEN = dict(gen1="gen1", gen2="gen2", gen3="gen3", mix="gen2")     # ... and the generation whose costs each solved


def _feasible_start(eng, slot, vlo, vup):
    """the standard basis and the feasibility LP (zero cost) in a slot: what an objective batch may start from"""
    eng.reset_slot(int(slot))
    st, _ = eng.solve_batch([slot], [slot], vlo, vup)
    assert st[0] == OPTIMAL, st


def _solve_obj(eng, src, dst, first, C, retry, vlo=None, vup=None):
    """one objective batch; retry (the revised form): an LP that comes back UNDEFINED is solved once more in its slot, reset and holding
    the feasibility solution again, as the header tells callers to.  Returns statuses, pivots and the number of retries."""
    st, it = eng.solve_batch_obj(src, dst, first, C, vlo, vup)
    st, it, n = st.copy(), it.copy(), 0
    if retry:
        for b in np.nonzero(st == UNDEFINED)[0]:
            one = slice(b, b + 1)
            _feasible_start(eng, dst[b], NONE if vlo is None else vlo[one], NONE if vup is None else vup[one])
            s1, i1 = eng.solve_batch_obj([dst[b]], [dst[b]], first, C[one], None if vlo is None else vlo[one], None if vup is None else vup[one])
            st[b], it[b], n = s1[0], it[b] + i1[0], n + 1
    return st, it, n


def _do_run(M, N, rng_name, form):
    s = lc.objective_set(M, N, rng_name)
    first, C1, C2, C3 = s["cost_first"], s["costs"]["gen1"], s["costs"]["gen2"], s["costs"]["gen3"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL, form)
    assert eng.rows_folded() == 0
    rec = dict(retries=0, primal_steps=0)
    _feasible_start(eng, 0, NONE, NONE)
    zeros = np.zeros(NLP, np.int32)

    def batch(name, src, dst, C, count=True):
        st, it, n = _solve_obj(eng, src, dst, first, C, retry and count)
        rec[name] = _read(eng, dst, st, it)
        rec["retries"] += n
        if n == 0:
            rec["primal_steps"] += eng.last_stats()["primal_steps"]

    batch("gen1", zeros, GEN1, C1)
    if form == "tableau":
        st, it = [], []
        for b in range(NLP):
            s1, i1 = eng.solve_batch_obj([0], [ALONE[b]], first, C1[b:b + 1])
            st.append(s1[0]); it.append(i1[0])
        rec["gen1_alone"] = _read(eng, ALONE, st, it)
        batch("gen1_sub", zeros[:SUB], SCRATCH[:SUB], C1[:SUB], count=False)
    batch("gen2", GEN1, GEN2, C2)
    if form == "tableau":
        st, it = [], []
        for b in range(NLP):
            s1, i1 = eng.solve_batch_obj([GEN1[b]], [SCRATCH[b]], first, C2[b:b + 1])
            st.append(s1[0]); it.append(i1[0])
        rec["gen2_alone"] = _read(eng, SCRATCH, st, it)
    batch("gen3", GEN2, GEN2, C3)
    batch("again", GEN2, GEN2, C3, count=False)
    src = np.where(np.arange(NLP) % 2 == 0, 0, GEN1).astype(np.int32)
    batch("mix", src, MIX, C2)
    eng.close()
    return rec


_RUNS = {}


def _run(M, N, rng_name, form):
    """every solve of one set in one form, once: the tests only look at the record"""
    key = (M, N, rng_name, form)
    if key not in _RUNS:
        _RUNS[key] = _do_run(M, N, rng_name, form)
    return _RUNS[key]


def _assert_against_references(s, folded, ref, oracle_gap, got, tag, lps=None):
    """statuses, objectives (both yardsticks) and the certificate, over all M + N variables and for the folded cost, of every LP of one
    batch that the yardsticks call OPTIMAL; returns the certificates"""
    certs = []
    for b, t in enumerate(range(len(ref)) if lps is None else lps):
        r = ref[t]
        assert got["st"][b] == r["st"], (tag, b, t, got["st"], [q["st"] for q in ref])
        if r["st"] != OPTIMAL:
            continue
        np.testing.assert_allclose(got["obj"][b], r["obj"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d" % (tag, t))
        np.testing.assert_allclose(got["obj"][b], r["obj_highs"], rtol=RTOL, atol=1e-9, err_msg="%s lp %d (HiGHS)" % (tag, t))
        c = lc.certify(s["A"], s["lo"], s["up"], folded[t], int(got["st"][b]), got["obj"][b], got["prim"][b], got["dual"][b])
        certs.append(c)
        lc.assert_certified(c, got["obj"][b], oracle_gap, (tag, b, t))
    return certs


def _report(form, M, N, what, certs, oracle, retries):
    w = lc.worst(certs)
    print("lp_obj_general_residuals engine %s M %d N %d %s lps %d retries %d rows %.3e feas %.3e dj %.3e side %.3e gap %.3e (oracle gap %.3e)" % (
        form, M, N, what, len(certs), retries, w["rows"], w["feas"], w["dj"], w["side"], w["gap"], oracle["gap"]))


def _check_run(M, N, rng_name, form):
    s = lc.objective_set(M, N, rng_name)
    ref, oracle, _ = lc.assert_objective_references_agree(M, N, rng_name)      # (the yardsticks agree: checked when the seeds were chosen)
    rec = _run(M, N, rng_name, form)
    tag = (form, M, N, rng_name)
    print("pivots %s: %s retries %d primal steps %d" % (tag, " ".join("%s %s" % (g, rec[g]["it"]) for g in BATCHES), rec["retries"], rec["primal_steps"]))
    assert rec["primal_steps"] > 0, tag          # (bslv_lpq_last_ext_stats: an objective batch works by primal steps, pivots and bound switches)
    certs = []
    for g in BATCHES:
        assert np.all(rec[g]["st"] == OPTIMAL), (tag, g, rec[g]["st"])
        certs += _assert_against_references(s, s["folded"][REF_GEN[g]], ref[REF_GEN[g]], oracle["gap"], rec[g], tag + (g,))
    _report(form, M, N, "range " + rng_name, certs, oracle, rec["retries"])
    # generation 3 again in place: an optimal slot is optimal for its own objective
    again, gen3 = rec["again"], rec["gen3"]
    assert np.all(again["st"] == OPTIMAL) and np.all(again["it"] == 0), (tag, again["st"], again["it"])
    np.testing.assert_allclose(again["obj"], gen3["obj"], rtol=RTOL, atol=1e-9)
    for k in ("prim", "dual"):          # (beta is recomputed at the start of a solve: 1e-8, the project's figure for a value against its bound)
        np.testing.assert_allclose(again[k], gen3[k], rtol=RTOL, atol=1e-8, err_msg=str(tag + (k,)))
    return rec


def _ranges(shapes):
    return [(M, N, r) for M, N in shapes for r in lc.obj_ranges(M, N)]


# ---- 1. the tableau form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rng_name", _ranges(SHAPES))
def test_objective_batches_on_a_general_set(oracle, M, N, rng_name):
    rec = _check_run(M, N, rng_name, "tableau")
    assert rec["retries"] == 0
    # a batch is its LPs alone, bit for bit: the batch of 16, its first 7, the second generation, the warm-started half of the mixed batch
    _assert_identical(rec["gen1"], rec["gen1_alone"], (M, N, rng_name, "16 against 1"))
    _assert_identical(rec["gen1"], rec["gen1_sub"], (M, N, rng_name, "16 against 7"), sel=slice(0, SUB))
    _assert_identical(rec["gen2"], rec["gen2_alone"], (M, N, rng_name, "second generation, 16 against 1"))
    odd = dict((k, v[1::2]) for k, v in rec["mix"].items())
    _assert_identical(rec["gen2"], odd, (M, N, rng_name, "mixed batch"), sel=slice(1, None, 2))


# ---- 2. the revised form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rng_name", _ranges(REV_SHAPES))
def test_objective_batches_in_the_revised_form_on_a_general_set(oracle, M, N, rng_name):
    rec = _check_run(M, N, rng_name, "revised")          # (all OPTIMAL after at most one retry each)
    tab = _run(M, N, rng_name, "tableau")
    for g in BATCHES:
        assert np.array_equal(rec[g]["st"], tab[g]["st"]), (M, N, rng_name, g, rec[g]["st"], tab[g]["st"])
        np.testing.assert_allclose(rec[g]["obj"], tab[g]["obj"], rtol=RTOL, atol=1e-9)


def test_price_vector_in_global_memory_on_a_general_set(oracle):
    """BSLV_REV_PRICE_LDS=0 (read per call): y of k_rev_price from global scratch (k_rev_y) instead of LDS, on two slices of columns that
    all carry a cost: the same values, bit for bit"""
    rec = {}
    for lds in ("1", "0"):
        with _env(BSLV_REV_PRICE_LDS=lds):
            rec[lds] = _do_run(24, 513, "cols", "revised")
    assert rec["1"]["retries"] == rec["0"]["retries"]
    for g in BATCHES + ("again",):
        _assert_identical(rec["1"][g], rec["0"][g], ("price vector", g))
        assert np.array_equal(rec["1"][g]["it"], rec["0"][g]["it"]), g


# ---- 3. a per-LP bound range under a new objective ------------------------------------------------------------------------------
BOUNDS_LP = 3
_BREF = {}


def _bounds_references(M, N, rng_name):
    """generation 1 of the objective set under the bounds of LP 3 of general_set(M, N, "a"): both yardsticks, asserted to agree"""
    key = (M, N, rng_name)
    if key not in _BREF:
        s, g = lc.objective_set(M, N, rng_name), lc.general_set(M, N, "a")
        lo, up = g["lps"][BOUNDS_LP]
        rows = lc._reference_rows(s["A"], lo, up, s["folded"]["gen1"])
        lc._assert_rows_agree(rows, (M, N, rng_name, "bounds of LP 3"))
        _BREF[key] = (rows, lc.worst([r["cert"] for r in rows]))
    return _BREF[key]


@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("rng_name", ["cols", "straddle"])
@pytest.mark.parametrize("M,N", SIDE_SHAPES)
def test_objective_batch_with_per_lp_bounds(oracle, M, N, rng_name, form):
    """the engine of general_set's arrangement "a" (var_first = 0, var_cnt = M: every row's bounds come per LP) with a zero cost; every
    LP of the objective batch has the bounds of that set's LP 3: LO / UP through vlo / vup under objmode ("straddle": on row variables
    that carry a cost as well)"""
    s, g = lc.objective_set(M, N, rng_name), lc.general_set(M, N, "a")
    ref, oracle_w = _bounds_references(M, N, rng_name)
    assert all(r["st"] == OPTIMAL for r in ref)
    lo, up = g["lps"][BOUNDS_LP]
    vlo, vup = np.tile(g["vlo"][BOUNDS_LP], (NLP, 1)), np.tile(g["vup"][BOUNDS_LP], (NLP, 1))
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], g["var_first"], g["var_cnt"], 1 + NLP, form)
    assert eng.rows_folded() == 0
    _feasible_start(eng, 0, vlo[:1], vup[:1])
    st, it, n = _solve_obj(eng, np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"]["gen1"], form == "revised", vlo, vup)
    got = _read(eng, GEN1, st, it)
    eng.close()
    print("pivots %s: %s retries %d" % ((form, M, N, rng_name, "bounds of LP 3"), got["it"], n))
    certs = _assert_against_references(dict(s, lo=lo, up=up), s["folded"]["gen1"], ref, oracle_w["gap"], got, (form, M, N, rng_name, "bounds of LP 3"))
    assert len(certs) == NLP
    _report(form, M, N, "range %s, bounds of LP 3" % rng_name, certs, oracle_w, n)


# ---- 4. unbounded objectives in a batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("M,N", SIDE_SHAPES)
def test_unbounded_objectives_in_a_mixed_batch(oracle, M, N, form):
    """a free column in no row: LPs 2, 5 and 9 put a cost on it and are UNBOUNDED; the others are what they are without those beside them"""
    s = lc.unbounded_objective_set(M, N)
    ref, oracle_w = lc.unbounded_objective_references(M, N)
    keep = np.array([t for t in range(NLP) if t not in lc.UNB_LPS])
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, 1 + 2 * NLP, form)
    _feasible_start(eng, 0, NONE, NONE)
    retry = form == "revised"
    st, it, n = _solve_obj(eng, np.zeros(NLP, np.int32), GEN1, s["cost_first"], s["costs"], retry)
    got = _read(eng, GEN1, st, it)
    st, it, n2 = _solve_obj(eng, np.zeros(len(keep), np.int32), ALONE[:len(keep)], s["cost_first"], s["costs"][keep], retry)
    without = _read(eng, ALONE[:len(keep)], st, it)
    eng.close()
    tag = (form, M, N, "unbounded objectives")
    print("pivots %s: %s retries %d" % (tag, got["it"], n + n2))
    assert [int(v) for v in got["st"]] == [UNBOUNDED if t in lc.UNB_LPS else OPTIMAL for t in range(NLP)], (tag, got["st"])
    certs = _assert_against_references(s, s["folded"], ref, oracle_w["gap"], got, tag)
    assert len(certs) == len(keep)
    _report(form, M, N, "unbounded objectives", certs, oracle_w, n + n2)
    _assert_identical(got, without, tag, sel=keep)


# ---- 5. the fill byte -------------------------------------------------------------------------------------------------------------
def _digest(rec):
    h = hashlib.sha256()
    for g in sorted(k for k in rec if isinstance(rec[k], dict)):
        for k in ("st", "it", "obj", "prim", "dual"):
            h.update(np.ascontiguousarray(rec[g][k]).tobytes())
    return h.hexdigest()


def _child():
    rec = _run(24, 1025, "cols", "tableau")
    print("fill %s statuses %s" % (os.environ.get("BSLV_FILL"), "".join(str(v) for g in BATCHES for v in rec[g]["st"])))
    print("sha256 " + _digest(rec))


def test_objective_batches_do_not_depend_on_the_fill_byte():
    """BSLV_FILL (read once per process) is the byte fresh device allocations are filled with: nothing an objective batch reads may be
    memory that nobody wrote.  One fresh child process per fill byte."""
    out = []
    for fill in ("0x7F", None):
        env = dict(os.environ)
        env.pop("BSLV_FILL", None)
        env.pop("BSLV_LP_REV", None)
        if fill:
            env["BSLV_FILL"] = fill
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
        assert "Memory access fault" not in p.stderr, "fill %s: %s" % (fill, p.stderr[-800:])
        assert p.returncode == 0, "fill %s: rc %d\n%s" % (fill, p.returncode, p.stderr[-1500:])      # (the first child that fails ends the test)
        lines = p.stdout.strip().splitlines()
        print(lines[-2])
        assert lines[-2].split()[:2] == ["fill", str(fill)] and lines[-2].split()[3] == str(OPTIMAL) * (len(BATCHES) * NLP), lines[-2]
        out.append(lines[-1])
    assert out[0].startswith("sha256 ") and out[0] == out[1], out


# ---- 6. the sets reach the thresholds in the number of pivots ----------------------------------------------------------------------
def test_pivot_counts_cover_the_bands(oracle):
    """KP = 6: a solve of 1 .. 6 pivots has one pass over its tableau, one of 7 .. 12 two; REFRESH_AFTER = 32: beyond it optimality is
    only declared on a recomputed beta.  Over the shapes together some OPTIMAL LP of an objective batch has to fall into each of the
    three bands."""
    counts = []
    for M, N, rng_name in _ranges(SHAPES):
        rec = _run(M, N, rng_name, "tableau")
        for g in BATCHES:
            counts += [int(i) for i, st in zip(rec[g]["it"], rec[g]["st"]) if st == OPTIMAL]
    counts = np.array(counts)
    edges = [0, 1, 7, 13, 33, 1 << 30]
    hist = [int(np.sum((counts >= a) & (counts < b))) for a, b in zip(edges[:-1], edges[1:])]
    print("lp_obj_general_residuals pivots of the OPTIMAL LPs: 0: %d, 1..6: %d, 7..12: %d, 13..32: %d, more than 32: %d (max %d)" % (*hist, counts.max()))
    assert hist[1] > 0 and hist[2] > 0 and hist[4] > 0, hist


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "child":
        _child()
