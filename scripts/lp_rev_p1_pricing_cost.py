"""What Devex pricing costs and saves in a PRIMAL batch of the REVISED LP form (bslv_lpq_solve_batch_method_priced), per call and in one
process -- the two cases of scripts/lp_rev_primal_cost.py:

  general   the (24, 4100) set of tests/lp_cases.py, arrangement "a": its 16 LPs as one cold batch from 16 reset slots in place
  S-mid     P2(0) of the bench's S-mid problem (1011 x 506) from the standard basis, the engine forced into the revised form

each under PRIMAL with the three rule pairs: default (both DANTZIG), primal Devex (DANTZIG, DEVEX), dual Devex (DEVEX, DANTZIG).  Per
pair: statuses, pivots, phase-1 iterations, rebuilds of the phase-1 pricing vector, lock-step rounds, tableau passes, both pricing
triples and the wall-clock ms of the stream-synchronised call (one warm-up, then `repetitions` runs: the median and all of them).
--lib PATH measures another build of the library (the parent commit's, say): one that lacks the call runs the default rule alone,
through bslv_lpq_solve_batch_method.  --period K sets bslv_lpq_set_refactor_period(K).  One JSON line per case.
usage: lp_rev_p1_pricing_cost.py [general|S-mid|both] [repetitions] [--lib PATH] [--period K]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BSLV_LP_REV"] = "1"          # read at create

ARGS = [a for a in sys.argv[1:]]
LIB = PERIOD = None
if "--lib" in ARGS:
    LIB = ARGS[ARGS.index("--lib") + 1]
    del ARGS[ARGS.index("--lib"):ARGS.index("--lib") + 2]
if "--period" in ARGS:
    PERIOD = int(ARGS[ARGS.index("--period") + 1])
    del ARGS[ARGS.index("--period"):ARGS.index("--period") + 2]
import bensolve_amd._lib as _lib
if LIB:
    _lib.LIB_PATH = os.path.abspath(LIB)
from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine
import lp_cases as lc

PRIMAL = 1
PAIRS = (("default", 0, 0), ("primal_devex", 0, 1), ("dual_devex", 1, 0))


def timed(eng, pair, slots, vlo, vup, reps, priced):
    _, dr, pr = pair
    runs = []
    for _ in range(reps + 1):
        for k in slots:
            eng.reset_slot(int(k))
        t0 = time.perf_counter()
        st, it = eng.solve_batch_method_priced(PRIMAL, dr, pr, slots, slots, vlo, vup) if priced else eng.solve_batch_method(PRIMAL, slots, slots, vlo, vup)
        runs.append((time.perf_counter() - t0) * 1e3)
    ls = eng.last_stats()
    return dict(statuses="".join(str(int(x)) for x in st), pivots=int(it.sum()), pivots_max=int(it.max()), phase1_lps=ls["phase1_lps"], phase1_iterations=ls["phase1_iterations"],
                d1_rebuilds=ls["phase1_rebuilds"], rounds=ls["lockstep_iters"], passes=int(ls["passes"]), primal_pricing=eng.last_primal_pricing_stats(), dual_pricing=eng.last_pricing_stats(),
                period=eng.last_period_stats() if PERIOD else None, total_ms_median=float(np.median(runs[1:] or runs)), total_ms_all=[round(x, 2) for x in (runs[1:] or runs)],
                obj=[float(x) for x in eng.obj(slots)])


def run_case(eng, out, slots, vlo, vup, reps):
    import ctypes
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
    priced = hasattr(eng.lib, "bslv_lpq_solve_batch_method_priced")
    out.update(library=LIB or "this build", priced_call=priced, period=PERIOD)
    if PERIOD:
        assert eng.set_refactor_period(PERIOD) == 0
    for pair in (PAIRS if priced else PAIRS[:1]):
        out[pair[0]] = timed(eng, pair, slots, vlo, vup, reps, priced)
    eng.close()
    print(json.dumps(out), flush=True)


def general(reps):
    M, N = 24, 4100
    s = lc.general_set(M, N, "a")
    eng = LpEngine(M, N, s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], lc.NLP)
    run_case(eng, dict(case="general set (24, 4100) a, 16 LPs cold in one batch", repetitions=reps), np.arange(lc.NLP, dtype=np.int32), s["vlo"], s["vup"], reps)


def smid(reps):
    prob = synth.CONFIGS["S-mid"]()
    m2 = P2Model(prob)
    eng = LpEngine.from_model(m2, pool_slots=2)
    out = dict(case="S-mid P2(0) cold, one LP, revised form", M=m2.M - eng.rows_folded(), N=m2.N, repetitions=reps)
    run_case(eng, out, np.zeros(1, np.int32), np.full((1, m2.r), -np.inf), m2.ub_for(np.zeros((1, prob["q"]))), reps)


if __name__ == "__main__":
    what = ARGS[0] if len(ARGS) > 0 else "both"
    reps = int(ARGS[1]) if len(ARGS) > 1 else 3
    if what in ("general", "both"):
        general(reps)
    if what in ("S-mid", "both"):
        smid(reps)
