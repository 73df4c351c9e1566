"""The r weighted-sum LPs of PART 1 of phase2_primal (bslv_algs.c:976-1018; bslv_benson_start) at the LP layer, under two methods:

  dual    as the driver runs them: every LP from the standard basis (the 'retry ladder' taken at once: freeing row j-1 leaves the
          previous basis dual infeasible, which the dual method reports UNDEFINED)
  repair  bslv_lpq_set_method(REPAIR): LP j starts from the optimal basis of LP j-1, in place; the engine's primal phase 1 takes
          what the dual simplex cannot start

Pivots per LP and wall-clock milliseconds per LP (stream-synchronised calls; median of the repetitions after one warm-up), one JSON
line.  usage: lp_method_part1.py [config] [repetitions]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine


def part1(eng, model, method):
    r = model.r
    eng.set_method(0 if method == "dual" else 2)
    vlo = np.full((1, r), -np.inf)
    rows = []
    eng.reset_slot(0)
    for j in range(r):
        vup = np.full((1, r), np.inf)
        vup[0, j] = 0.0
        t0 = time.perf_counter()
        if method == "dual" and j > 0:
            eng.reset_slot(0)
        st, it = eng.solve_batch([0], [0], vlo, vup)
        ms = (time.perf_counter() - t0) * 1e3
        s = eng.last_stats()
        rows.append(dict(status=int(st[0]), pivots=int(it[0]), ms=ms, obj=float(eng.obj([0])[0]), phase1_iterations=s["phase1_iterations"], phase1_lps=s["phase1_lps"]))
    return rows


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-small"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    model = P2Model(synth.CONFIGS[name]())
    eng = LpEngine.from_model(model, pool_slots=2)
    out = dict(config=name, M=model.M, N=model.N, r=model.r, repetitions=reps)
    for method in ("dual", "repair"):
        runs = [part1(eng, model, method) for _ in range(reps + 1)][1:]
        first = runs[0]
        out[method] = dict(status=[x["status"] for x in first], pivots_per_lp=[x["pivots"] for x in first], phase1_iterations=[x["phase1_iterations"] for x in first],
                           obj=[x["obj"] for x in first],
                           ms_per_lp_median=[float(np.median([run[j]["ms"] for run in runs])) for j in range(model.r)],
                           ms_total_median=float(np.median([sum(x["ms"] for x in run) for run in runs])),
                           ms_total_min_max=[float(min(sum(x["ms"] for x in run) for run in runs)), float(max(sum(x["ms"] for x in run) for run in runs))])
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
