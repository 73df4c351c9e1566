"""Pivots, passes and milliseconds of the LP engine's PRIMAL steps under the two rules of bslv_lpq_set_primal_pricing (0 largest
reduced-cost violation, 1 primal Devex) at the LP layer, both rules in one process:

  part1   the weighted-sum LPs P1(w) that open the dual Benson variant -- the q unit weights and the central one -- as one objective
          batch (bslv_lpq_solve_batch_obj) from the feasibility basis in slot 0
  far     a batch of B objective LPs warm-started far from their parent: the parent is P1(w) of the central weight, the children have
          random weights from the whole simplex (ex09: from the dual of its ordering cone)
  cold    P2(v) from the standard basis under BSLV_LP_METHOD_PRIMAL (phase 1, then the primal phase 2)          [S-mid only]

P1(w): min w.y, rows of the problem, -P x + y = 0 (tests/test_lp_rev_obj_gpu.py's P1Model).  Per rule: statuses, pivots, tableau
passes, wall-clock ms of the stream-synchronised call (median of the repetitions after one warm-up), the counters of
bslv_lpq_last_primal_pricing_stats, the largest relative difference of the optimal values between the rules.  One JSON line.
usage: lp_primal_pricing_probe.py [S-mid|S-degenerate|ex09] [repetitions] [B]     (ex09: BSLV_LP_REV=1 is set, the revised form)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine
from test_lp_rev_obj_gpu import P1Model

NONE = np.zeros((1, 0))
PRIMAL, REPAIR = 1, 2


def timed_obj(eng, src, dst, first, C, reps):
    runs = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        st, it = eng.solve_batch_obj(src, dst, first, C)
        runs.append((time.perf_counter() - t0) * 1e3)
    ls = eng.last_stats()
    return dict(optimal=int((st == 4).sum()), lps=len(st), statuses="".join(str(int(x)) for x in st), pivots_total=int(it.sum()), pivots_per_lp=[int(x) for x in it] if len(it) <= 16 else None,
                pivots_max=int(it.max()), passes=int(ls["passes"]), ms_median=float(np.median(runs[1:])), ms_all=[round(x, 2) for x in runs[1:]],
                pricing=eng.last_primal_pricing_stats()), eng.obj(dst)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-mid"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    if name == "ex09":
        os.environ.setdefault("BSLV_LP_REV", "1")
        prob = synth.read_vlp(os.path.join(ROOT, "tests", "golden", "ex", "ex09.vlp"))
    else:
        prob = synth.CONFIGS[name]()
    q = prob["q"]
    model = P1Model(prob)
    eng = model.engine(B + q + 2)
    out = dict(config=name, M=model.M - eng.rows_folded(), N=model.N, q=q, repetitions=reps, batch=B)
    # the feasibility basis under REPAIR (the extended selection, with its cost perturbation): at S-mid size the zero-cost LP is so
    # dual degenerate that the default method's plain selection runs into the iteration limit (76 500 pivots, UNDEFINED)
    if not os.environ.get("BSLV_LP_REV"):
        assert eng.set_method(REPAIR) == 0
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], NONE, NONE)
    out["feasibility"] = dict(method="repair" if not os.environ.get("BSLV_LP_REV") else "dual", status=int(st[0]), pivots=int(it[0]))
    if st[0] != 4 and not os.environ.get("BSLV_LP_REV"):
        # ... and where that fails too (S-degenerate), phase 1 of the PRIMAL method under the rule this probe is about
        assert eng.set_method(PRIMAL) == 0 and eng.set_primal_pricing(1) == 0
        eng.reset_slot(0)
        t0 = time.perf_counter()
        st, it = eng.solve_batch([0], [0], NONE, NONE)
        out["feasibility_fallback"] = dict(method="primal, primal Devex", status=int(st[0]), pivots=int(it[0]), ms=(time.perf_counter() - t0) * 1e3)
    assert st[0] == 4, out
    if not os.environ.get("BSLV_LP_REV"):
        assert eng.set_method(0) == 0
    rng = np.random.default_rng(0)
    if prob.get("gen") is not None and prob.get("cone_kind") == 1:
        # an ordering cone given by generators (ex09, q = 3): P1(w) is bounded for the weights of its dual cone only, whose extreme rays are
        # the cross products of two generators that no generator contradicts; the weights are convex combinations of the rays
        assert q == 3
        G = prob["gen"] / np.linalg.norm(prob["gen"], axis=0, keepdims=True)
        rays = []
        for i in range(G.shape[1]):
            for j in range(i + 1, G.shape[1]):
                for sgn in (1.0, -1.0):
                    w = sgn * np.cross(G[:, i], G[:, j])
                    if np.linalg.norm(w) > 1e-12 and (w @ G).min() >= -1e-12:
                        rays.append(w / np.abs(w).sum())
        rays = np.array(rays)
        assert len(rays) >= 3, rays
        mix = lambda n: (rng.dirichlet(np.full(len(rays), 0.5), size=n) * 0.9 + 0.1 / len(rays)) @ rays
        central = rays.mean(axis=0, keepdims=True)
        W1, WB = np.vstack([mix(q), central]), mix(B)
        out["weights"] = "convex combinations of the %d extreme rays of the dual cone of the %d generators" % (len(rays), G.shape[1])
    else:
        central = np.full((1, q), 1.0 / q)
        W1 = np.vstack([np.eye(q) * 0.96 + 0.04 / q, central])          # (the unit weights, kept inside the simplex)
        WB = rng.dirichlet(np.full(q, 0.5), size=B) * 0.96 + 0.04 / q
    objs = {}
    for rule, key in ((0, "dantzig"), (1, "devex")):
        assert eng.set_primal_pricing(rule) == 0
        rec = {}
        n1 = len(W1)
        rec["part1"], o1 = timed_obj(eng, np.zeros(n1, np.int32), np.arange(1, n1 + 1, dtype=np.int32), model.y_first, W1, reps)
        parent = n1                       # the central weight's slot
        rec["far"], o2 = timed_obj(eng, np.full(B, parent, np.int32), np.arange(n1 + 1, n1 + 1 + B, dtype=np.int32), model.y_first, WB, reps)
        objs[key] = np.concatenate([o1, o2])
        out[key] = rec
    eng.close()
    out["max_rel_obj_diff"] = float(np.max(np.abs(objs["dantzig"] - objs["devex"]) / (1 + np.abs(objs["dantzig"]))))
    if name == "S-mid":
        m2 = P2Model(prob)
        e2 = LpEngine.from_model(m2, pool_slots=2)
        assert e2.set_method(PRIMAL) == 0
        free = np.full((1, m2.r), -np.inf)
        for rule, key in ((0, "dantzig"), (1, "devex")):
            assert e2.set_primal_pricing(rule) == 0
            runs = []
            for _ in range(reps + 1):
                e2.reset_slot(0)
                t0 = time.perf_counter()
                st, it = e2.solve_batch([0], [0], free, m2.ub_for(np.zeros((1, q))))
                runs.append((time.perf_counter() - t0) * 1e3)
            ls = e2.last_stats()
            out[key]["cold"] = dict(status=int(st[0]), pivots=int(it[0]), passes=int(ls["passes"]), phase1_iterations=int(ls["phase1_iterations"]), ms_median=float(np.median(runs[1:])),
                                    ms_all=[round(x, 2) for x in runs[1:]], obj=float(e2.obj([0])[0]), pricing=e2.last_primal_pricing_stats())
        e2.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
