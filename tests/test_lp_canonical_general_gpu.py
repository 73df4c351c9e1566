"""GPU: canonical optimal duals of the LP engine (bslv_lpq_set_canonical, tie_once / k_select_tie of bensolve_amd/csrc/lp_engine.hip)
on GENERAL models -- the branches of the tie phase that a P2(v) model (tests/test_lp_canonical_gpu.py) cannot reach: a tie on a LOWER
bound (`below`), a tied BASIC per-LP variable whose own bound moves (tie_shift), a per-LP column that enters (`sq`), free nonbasic
variables (the NS_F skip), boxed and fixed variables, and the exit without an entering candidate (Tv.stat[2]).

The cases, their directions and the EXPECTED canonical dual -- the full dual vector, M + N entries, that HiGHS gives the LP with its
per-LP bounds moved by t d at t = 2^-10 and 2^-11 -- are tests/canonical_general_cases.py's; `python
tests/canonical_general_cases.py` and tests/test_lp_canonical_general_cases.py show without a GPU that every set meets its conditions.

Shapes (lp_cases.general_set, both arrangements): (15, 16) (16, 17): ld = 16 against 32 (raw_create, "L.ld = (N + 15) / 16 * 16");
(31, 64) (32, 65): one wave of 64 columns against two, M + 1 = 32 against 33.  The widths beyond are tests/test_lp_canonical_gpu.py's
wide sets: the general sets from (33, 257) on have no degenerate tie under this construction.

A run (the protocol of test_lp_canonical_gpu.py): LP 0 of the set cold into slot 0 with the switch off, then every kept LP from slot 0
in one batch -- once on an engine with the switch off, once on one with it on; on that one also every LP alone from slot 0, and a second
generation (LP perm[b] from the slot of LP b, where both are kept) that is then solved again in place.

Exit sets (arrangement "a", the mixed-sign direction; (16, 17), (32, 65) and (24, 1536), where the selection runs NT_BIG threads):
HiGHS calls the shifted LP of every OPTIMAL LP infeasible at both t.  A basis without a wrong tied row would stay primal feasible for
small t > 0, so every one of these LPs has to leave the phase where the ratio test finds no entering candidate -- or at the cap, which
the test forbids."""
import numpy as np
import pytest

import canonical_general_cases as cg
import lp_cases as lc
from bensolve_amd.lp import LpEngine
from lp_cases import OPTIMAL, INFEASIBLE, NLP

pytestmark = pytest.mark.gpu
RTOL = 1e-9               # tests/test_lp_canonical_gpu.py's bounds against HiGHS
ZERO = dict(entered=0, tie_pivots=0, no_candidate=0, capped=0)
SETS = [(M, N, arr) for M, N in cg.SHAPES for arr in ("a", "b")]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _read(eng, dst, st, it):
    n = eng.M + eng.N
    return dict(st=np.array(st), it=np.array(it), obj=eng.obj(dst), prim=eng.primal(dst, 0, n), dual=eng.dual(dst, 0, n), canon=eng.last_canonical_stats())


def _start(c, slots, on):
    """an engine of its own with LP 0 of the set solved cold into slot 0, the switch off; then the switch as asked"""
    eng = LpEngine(c["M"], c["N"], c["A"], c["lo"], c["up"], c["cost"], c["var_first"], c["var_cnt"], slots)
    eng.reset_slot(0)
    st0, _ = eng.solve_batch([0], [0], c["vlo0"][None], c["vup0"][None])
    assert st0[0] == OPTIMAL
    if on:
        assert eng.set_canonical(1, c["dir"]) == 0 and eng.get_canonical() == 1
    return eng


_RUNS = {}


def _run(M, N, arr):
    """every solve of one set, once: the tests only look at the record"""
    key = (M, N, arr)
    if key in _RUNS:
        return _RUNS[key]
    c = cg.tied_set(M, N, arr)
    cg.check_tied_set(c)
    vlo, vup, B = c["vlo"], c["vup"], len(c["lps"])
    batch, alone, gen2 = (np.arange(1 + k * B, 1 + (k + 1) * B, dtype=np.int32) for k in range(3))
    rec = {}
    for on in (0, 1):
        eng = _start(c, 1 + 3 * B, on)
        st, it = eng.solve_batch(np.zeros(B, np.int32), batch, vlo, vup)
        rec[on] = _read(eng, batch, st, it)
        if on:
            st, it = [], []
            for b in range(B):
                s1, i1 = eng.solve_batch([0], [alone[b]], vlo[b:b + 1], vup[b:b + 1])
                st.append(s1[0]); it.append(i1[0])
            rec["alone"] = _read(eng, alone, st, it)
            # the second generation: LP perm[lps[b]] from the slot of LP lps[b], where the keep rule kept both
            where = {int(t): j for j, t in enumerate(c["lps"])}
            pairs = [(b, where[int(c["perm"][t])]) for b, t in enumerate(c["lps"]) if int(c["perm"][t]) in where]
            src, tgt = np.array([batch[b] for b, _ in pairs], np.int32), np.array([j for _, j in pairs])
            st, it = eng.solve_batch(src, gen2[:len(pairs)], vlo[tgt], vup[tgt])
            rec["gen2"] = dict(_read(eng, gen2[:len(pairs)], st, it), lps=tgt)
            st, it = eng.solve_batch(gen2[:len(pairs)], gen2[:len(pairs)], vlo[tgt], vup[tgt])
            rec["again"] = _read(eng, gen2[:len(pairs)], st, it)
        eng.close()
    _RUNS[key] = rec
    return rec


def _moved(c, off):
    """degenerate cases whose off-solve gave another dual than the expected one"""
    return int((c["degenerate"] & (np.abs(off["dual"] - c["dual"]).max(axis=1) > 1e-6)).sum())


@pytest.mark.parametrize("M,N,arr", SETS)
def test_switch_on_returns_the_dual_of_the_shifted_lp(oracle, M, N, arr):
    c = cg.tied_set(M, N, arr)
    oracle_gap = lc.general_references(M, N, arr)[1]["gap"]
    rec = _run(M, N, arr)
    off, on = rec[0], rec[1]
    print("lp_canonical_shapes general M %d N %d arr %s: %d cases, %d degenerate; off-solve differs from the canonical dual in %d; largest |dual - expected| "
          "with the switch on %.3e; tie phase %s" % (M, N, arr, len(c["lps"]), int(c["degenerate"].sum()), int((np.abs(off["dual"] - c["dual"]).max(axis=1) > 1e-6).sum()),
                                                     np.abs(on["dual"] - c["dual"]).max(), on["canon"]))
    assert np.all(off["st"] == OPTIMAL)
    assert np.array_equal(on["st"], off["st"])
    assert _same_bits(on["obj"], off["obj"]), "the objective changed with the switch: %s" % (on["obj"] - off["obj"])
    assert _same_bits(on["prim"], off["prim"]), "primal values changed with the switch"      # (a tie pivot is a step of length zero)
    np.testing.assert_allclose(off["obj"], c["z"], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(on["dual"], c["dual"], rtol=RTOL, atol=1e-9)
    for b, t in enumerate(c["lps"]):
        lo, up = c["bounds"][b]
        cert = lc.certify(c["A"], lo, up, c["cost"], int(on["st"][b]), on["obj"][b], on["prim"][b], on["dual"][b])
        lc.assert_certified(cert, on["obj"][b], oracle_gap, (M, N, arr, t))


@pytest.mark.parametrize("M,N,arr", SETS)
def test_the_counters_of_the_tie_phase(oracle, M, N, arr):
    c = cg.tied_set(M, N, arr)
    rec = _run(M, N, arr)
    moved = _moved(c, rec[0])
    print("lp_canonical_shapes general M %d N %d arr %s: %d degenerate cases whose off-solve gave another dual; %s" % (M, N, arr, moved, rec[1]["canon"]))
    assert rec[1]["canon"]["entered"] >= moved and rec[1]["canon"]["entered"] <= len(c["lps"])
    assert rec[1]["canon"]["capped"] == 0
    assert rec[0]["canon"] == ZERO


def test_some_off_solve_differs_from_the_canonical_dual(oracle):
    """over the required sets together: without it no case would show what the switch is for"""
    differ = {k: int((np.abs(_run(*k)[0]["dual"] - cg.tied_set(*k)["dual"]).max(axis=1) > 1e-6).sum()) for k in SETS if k[:2] in cg.REQUIRED}
    pivots = {k: _run(*k)[1]["canon"]["tie_pivots"] for k in differ}
    print("lp_canonical_shapes general: cases whose off-solve gave another dual %s; tie pivots %s" % (differ, pivots))
    assert sum(differ.values()) > 0
    assert sum(pivots.values()) >= sum(differ.values())            # (a basis changes by pivots only)


@pytest.mark.parametrize("M,N,arr", SETS)
def test_a_batch_is_its_lps_alone(oracle, M, N, arr):
    """the tie phase compacts its list of active LPs and doubles its chunk of rounds: neither may show in a result"""
    rec = _run(M, N, arr)
    for k in ("st", "obj", "prim", "dual"):
        assert _same_bits(rec[1][k], rec["alone"][k]), (M, N, arr, k, rec[1]["it"], rec["alone"]["it"])


@pytest.mark.parametrize("M,N,arr", SETS)
def test_second_generation_reaches_the_same_dual(oracle, M, N, arr):
    c = cg.tied_set(M, N, arr)
    rec = _run(M, N, arr)
    gen2, again = rec["gen2"], rec["again"]
    tgt = gen2["lps"]
    assert len(tgt) >= len(c["lps"]) // 2, "too few pairs of kept LPs"
    print("lp_canonical_shapes general M %d N %d arr %s: second generation of %d LPs, largest |dual - expected| %.3e, tie phase %s; again in place: pivots %s" % (
        M, N, arr, len(tgt), np.abs(gen2["dual"] - c["dual"][tgt]).max(), gen2["canon"], again["it"]))
    assert np.all(gen2["st"] == OPTIMAL)
    np.testing.assert_allclose(gen2["obj"], c["z"][tgt], rtol=RTOL, atol=1e-9)
    np.testing.assert_allclose(gen2["dual"], c["dual"][tgt], rtol=RTOL, atol=1e-9)
    assert gen2["canon"]["capped"] == 0
    assert np.all(again["st"] == OPTIMAL) and np.all(again["it"] == 0), again["it"]
    np.testing.assert_allclose(again["dual"], c["dual"][tgt], rtol=RTOL, atol=1e-9)


@pytest.mark.parametrize("M,N", cg.EXIT_SHAPES)
def test_exit_without_an_entering_candidate(oracle, M, N):
    e = cg.exit_set(M, N)
    assert all(st == (INFEASIBLE, INFEASIBLE) for st in e["shifted_status"]), e["shifted_status"]
    ref, worst = lc.assert_references_agree(M, N, "a")
    dst = np.arange(1, NLP + 1, dtype=np.int32)
    rec = {}
    for on in (0, 1):
        eng = _start(e, NLP + 1, on)
        st, it = eng.solve_batch(np.zeros(NLP, np.int32), dst, e["vlo"], e["vup"])
        rec[on] = _read(eng, dst, st, it)
        eng.close()
    off, on = rec[0], rec[1]
    opt = e["optimal"]
    print("lp_canonical_shapes exit M %d N %d: %d OPTIMAL LPs of %d; tie phase %s; pivots off %s on %s" % (M, N, int(opt.sum()), NLP, on["canon"], off["it"], on["it"]))
    assert [int(s) for s in off["st"]] == [r["st"] for r in ref]
    assert np.array_equal(on["st"], off["st"]) and np.array_equal(on["st"] == OPTIMAL, opt)
    assert _same_bits(on["obj"][opt], off["obj"][opt]) and _same_bits(on["prim"][opt], off["prim"][opt])
    np.testing.assert_allclose(on["obj"][opt], e["z"][opt], rtol=RTOL, atol=1e-9)
    for t in np.nonzero(opt)[0]:
        lo, up = e["bounds"][t]
        cert = lc.certify(e["A"], lo, up, e["cost"], int(on["st"][t]), on["obj"][t], on["prim"][t], on["dual"][t])
        lc.assert_certified(cert, on["obj"][t], worst["gap"], (M, N, "exit", t))
    assert off["canon"] == ZERO
    assert on["canon"]["capped"] == 0
    assert on["canon"]["entered"] == int(opt.sum())
    assert on["canon"]["no_candidate"] == int(opt.sum()), on["canon"]
