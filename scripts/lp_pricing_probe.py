"""Pivots and milliseconds of the LP engine under its two pricing rules (bslv_lpq_set_pricing: 0 largest violation, 1 dual Devex) on
the LPs of a synthetic config, at the LP layer:

  cold    P2(v) from the standard basis (what bslv_benson_start and every retry from a reset slot do)
  part1   the r weighted-sum LPs of PART 1 of phase2_primal (bslv_algs.c:976-1018), each from the standard basis as the driver runs them
  warm    a batch of B P2(v) solves warm-started from the cold LP's slot, right-hand sides near its boundary point (scripts/lp_probe.py)

Per rule: statuses, pivots per LP, wall-clock ms (stream-synchronised calls; median of the repetitions after one warm-up), the
counters of bslv_lpq_last_pricing_stats.  One JSON line.  usage: lp_pricing_probe.py [config] [repetitions] [B]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine


def timed(eng, src, dst, vlo, vup):
    t0 = time.perf_counter()
    st, it = eng.solve_batch(src, dst, vlo, vup)
    ms = (time.perf_counter() - t0) * 1e3
    return st, it, ms, eng.last_pricing_stats(), eng.last_stats()


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-mid"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    prob = synth.CONFIGS[name]()
    model = P2Model(prob)
    q, r = prob["q"], model.r
    eng = LpEngine.from_model(model, pool_slots=B + 1)
    out = dict(config=name, M=model.M - eng.rows_folded(), N=model.N, r=r, repetitions=reps, batch=B)
    free = np.full((1, r), -np.inf)
    rng = np.random.default_rng(0)
    noise = np.abs(rng.normal(size=(B, q)))
    for rule, key in ((0, "dantzig"), (1, "devex")):
        assert eng.set_pricing(rule) == 0
        rec = {}
        runs = []
        for _ in range(reps + 1):
            eng.reset_slot(0)
            st, it, ms, ps, ls = timed(eng, [0], [0], free, model.ub_for(np.zeros((1, q))))
            runs.append(ms)
        rec["cold"] = dict(status=int(st[0]), pivots=int(it[0]), passes=ls["passes"], ms_median=float(np.median(runs[1:])), ms_all=[round(x, 2) for x in runs[1:]], obj=float(eng.obj([0])[0]), pricing=ps)
        y0 = eng.primal([0], model.y_first, q)[0]
        # warm batch from the cold LP's slot (the slot is this rule's own optimum: what the driver would start from)
        V = y0[None, :] - noise * 0.1 * np.abs(y0).mean()
        src, dst = np.zeros(B, np.int32), np.arange(1, B + 1, dtype=np.int32)
        runs = []
        for _ in range(reps + 1):
            st, it, ms, ps, ls = timed(eng, src, dst, np.full((B, r), -np.inf), model.ub_for(V))
            runs.append(ms)
        rec["warm"] = dict(optimal=int((st == 4).sum()), pivots_mean=float(it.mean()), pivots_max=int(it.max()), pivots_total=int(it.sum()), ms_median=float(np.median(runs[1:])), ms_all=[round(x, 2) for x in runs[1:]], pricing=ps)
        # PART 1: row j of the range bounded above by 0, the others free; every LP from the standard basis
        rows = []
        for rep in range(reps + 1):
            cur = []
            for j in range(r):
                vup = np.full((1, r), np.inf)
                vup[0, j] = 0.0
                eng.reset_slot(0)
                st, it, ms, ps, ls = timed(eng, [0], [0], free, vup)
                cur.append(dict(status=int(st[0]), pivots=int(it[0]), ms=ms, other_row=ps["other_row"]))
            rows.append(cur)
        rows = rows[1:]
        rec["part1"] = dict(status=[x["status"] for x in rows[0]], pivots_per_lp=[x["pivots"] for x in rows[0]], other_row=[x["other_row"] for x in rows[0]],
                            ms_per_lp_median=[float(np.median([run[j]["ms"] for run in rows])) for j in range(r)])
        out[key] = rec
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
