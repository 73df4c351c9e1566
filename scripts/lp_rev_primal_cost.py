"""What the simplex method costs in the REVISED LP form (bslv_lpq_solve_batch_method: DUAL, PRIMAL, REPAIR), per call and in one process:

  general   the (24, 4100) set of tests/lp_cases.py, arrangement "a": its 16 LPs as one cold batch from 16 reset slots in place
  S-mid     P2(0) of the bench's S-mid problem (1011 x 506) from the standard basis, the engine forced into the revised form

Per method: statuses, pivots, phase-1 LPs / iterations / rebuilds of the phase-1 pricing vector, lock-step rounds, tableau passes and
the wall-clock ms of the stream-synchronised call (one warm-up, then `repetitions` runs: the median and all of them).  With
BSLV_REV_PROBE=8 in the environment the library prints, per call, LP 0's clock ticks in the rebuilds of the phase-1 pricing vector
(stderr); the share of the call is that time over the call's ms.  One JSON line per case.
usage: lp_rev_primal_cost.py [general|S-mid|both] [repetitions]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BSLV_LP_REV"] = "1"          # read at create
from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine
import lp_cases as lc

METHODS = (("dual", 0), ("primal", 1), ("repair", 2))


def timed(eng, method, slots, vlo, vup, reps):
    runs = []
    for _ in range(reps + 1):
        for k in slots:
            eng.reset_slot(int(k))
        t0 = time.perf_counter()
        st, it = eng.solve_batch_method(method, slots, slots, vlo, vup)
        runs.append((time.perf_counter() - t0) * 1e3)
    ls = eng.last_stats()
    return dict(statuses="".join(str(int(x)) for x in st), pivots=int(it.sum()), pivots_max=int(it.max()), phase1_lps=ls["phase1_lps"], phase1_iterations=ls["phase1_iterations"],
                d1_rebuilds=ls["phase1_rebuilds"], rounds=ls["lockstep_iters"], passes=int(ls["passes"]), total_ms_median=float(np.median(runs[1:] or runs)), total_ms_all=[round(x, 2) for x in (runs[1:] or runs)],
                obj=[float(x) for x in eng.obj(slots)])


def is_revised(eng):
    import ctypes
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    return eng.lib.bslv_lpq_is_revised(eng.h) == 1


def general(reps):
    M, N = 24, 4100
    s = lc.general_set(M, N, "a")
    eng = LpEngine(M, N, s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], lc.NLP)
    assert is_revised(eng)
    out = dict(case="general set (24, 4100) a, 16 LPs cold in one batch", repetitions=reps)
    for name, m in METHODS:
        out[name] = timed(eng, m, np.arange(lc.NLP, dtype=np.int32), s["vlo"], s["vup"], reps)
    eng.close()
    print(json.dumps(out), flush=True)


def smid(reps):
    prob = synth.CONFIGS["S-mid"]()
    m2 = P2Model(prob)
    eng = LpEngine.from_model(m2, pool_slots=2)
    assert is_revised(eng)
    out = dict(case="S-mid P2(0) cold, one LP, revised form", M=m2.M - eng.rows_folded(), N=m2.N, repetitions=reps)
    free, ub = np.full((1, m2.r), -np.inf), m2.ub_for(np.zeros((1, prob["q"])))
    for name, m in METHODS:
        out[name] = timed(eng, m, np.zeros(1, np.int32), free, ub, reps)
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    if what in ("general", "both"):
        general(reps)
    if what in ("S-mid", "both"):
        smid(reps)
