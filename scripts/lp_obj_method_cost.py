"""Pivots and milliseconds of objective batches under PRIMAL, DUAL and REPAIR (bslv_lpq_solve_batch_obj_method) on the two S-mid
workloads of scripts/lp_primal_pricing_probe.py, in one process:

  part1   the weighted-sum LPs P1(w) that open the dual Benson variant -- the q unit weights and the central one -- as one objective
          batch from the feasibility basis in slot 0
  far     64 objective LPs warm-started far from their parent: the parent is P1(w) of the central weight (its PRIMAL solve), the
          children have random weights from the whole simplex

Per method one warm-up call and ONE timed one (host wall clock of the stream-synchronised call), the statuses, the pivots, the counters
of bslv_lpq_last_obj_method_stats and the largest relative difference of the optimal values against PRIMAL.  A library without the
call (the parent commit) gives the PRIMAL row alone, through bslv_lpq_solve_batch_obj.  One JSON line.
usage: lp_obj_method_cost.py [S-mid] [B]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bensolve_amd import synth, load_library
from test_lp_rev_obj_gpu import P1Model

NONE = np.zeros((1, 0))
DUAL, PRIMAL, REPAIR = 0, 1, 2


def timed(eng, method, src, dst, first, C):
    for k in range(2):      # (a warm-up, then the run that counts)
        t0 = time.perf_counter()
        st, it = eng.solve_batch_obj(src, dst, first, C) if method is None else eng.solve_batch_obj_method(method, src, dst, first, C)
        ms = (time.perf_counter() - t0) * 1e3
    ls = eng.last_stats()
    row = dict(statuses="".join(str(int(x)) for x in st), optimal=int((st == 4).sum()), lps=len(st), pivots=int(it.sum()), pivots_max=int(it.max()),
               passes=int(ls["passes"]), primal_steps=int(ls["primal_steps"]), ms=round(ms, 2))
    if method is not None:
        row["obj_method_stats"] = eng.last_obj_method_stats()
    return row, st, eng.obj(dst)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-mid"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    has_call = hasattr(load_library(), "bslv_lpq_solve_batch_obj_method")
    prob = synth.CONFIGS[name]()
    q = prob["q"]
    model = P1Model(prob)
    eng = model.engine(B + q + 2)
    out = dict(config=name, M=model.M - eng.rows_folded(), N=model.N, q=q, batch=B, has_call=has_call)
    assert eng.set_method(REPAIR) == 0      # (the feasibility LP: see lp_primal_pricing_probe.py)
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], NONE, NONE)
    assert st[0] == 4, st
    assert eng.set_method(0) == 0
    rng = np.random.default_rng(0)
    central = np.full((1, q), 1.0 / q)
    W1 = np.vstack([np.eye(q) * 0.96 + 0.04 / q, central])
    WB = rng.dirichlet(np.full(q, 0.5), size=B) * 0.96 + 0.04 / q
    n1 = len(W1)
    d1, dB = np.arange(1, n1 + 1, dtype=np.int32), np.arange(n1 + 1, n1 + 1 + B, dtype=np.int32)
    ref = {}
    # PRIMAL last for part1: the far batch starts from the slot its central LP leaves
    order = [("primal", PRIMAL if has_call else None)] if not has_call else [("dual", DUAL), ("repair", REPAIR), ("primal", PRIMAL)]
    rows = {}
    for key, m in order:
        rows[key] = dict(part1=timed(eng, m, np.zeros(n1, np.int32), d1, model.y_first, W1))
    ref["part1"] = rows["primal"]["part1"]
    for key, m in reversed(order):      # (every far batch starts from the central slot as PRIMAL's part1, the last one, left it)
        rows[key]["far"] = timed(eng, m, np.full(B, n1, np.int32), dB, model.y_first, WB)
    ref["far"] = rows["primal"]["far"]
    for key in rows:
        rec = {}
        for part in ("part1", "far"):
            row, st, obj = rows[key][part]
            ok = (st == 4) & (ref[part][1] == 4)
            row["max_rel_obj_diff_vs_primal"] = float(np.max(np.abs(obj[ok] - ref[part][2][ok]) / (1 + np.abs(ref[part][2][ok])))) if ok.any() else None
            rec[part] = row
        out[key] = rec
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
