"""Probe: one batch of P1(w) LPs (the LPs of the dual Benson variant: min w.y, A x >= 1, -P x + y = 0, x >= 0) through
bslv_lpq_solve_batch_obj in the tableau form (BSLV_LP_REV=0) and the revised form (=1): pivots, tableau passes and ms per batch.
The chain is dual_benson's: feasibility LP in slot 0, PART 1 in place, then B weights from slot 0 (timed, median of `reps`).
usage: p1_batch_forms.py sparse|covering m n q seed B reps [dense_cols]   -> one JSON line per form"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import numpy as np
from bensolve_amd import synth
from test_lp_rev_obj_gpu import P1Model, _sparse_covering

kind = sys.argv[1]
m, n, q, seed, B, reps = [int(x) for x in sys.argv[2:8]]
dense = int(sys.argv[8]) if len(sys.argv) > 8 else 0
prob = _sparse_covering(m, n, q, seed, dense_cols=dense) if kind == "sparse" else synth.covering_vlp(m, n, q, seed)
model = P1Model(prob)
rng = np.random.default_rng(seed)
W = rng.uniform(0.1, 1.0, size=(B, q))
W /= W.sum(axis=1, keepdims=True)
ref = None
for rev in ("0", "1"):
    os.environ["BSLV_LP_REV"] = rev
    eng = model.engine(B + 1)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
    assert st[0] == 4
    st, _ = eng.solve_batch_obj([0], [0], model.y_first, np.full((1, q), 1.0 / q))
    assert st[0] == 4
    src, dst = np.zeros(B, np.int32), np.arange(1, B + 1, dtype=np.int32)
    ms, wall = [], []
    for r in range(reps):
        t0 = time.perf_counter()
        st, it = eng.solve_batch_obj(src, dst, model.y_first, W)
        wall.append((time.perf_counter() - t0) * 1e3)
        s = eng.last_stats()
        ms.append(s["total_ms"])
    assert np.all(st == 4), st
    obj = eng.obj(dst)
    if ref is None:
        ref = obj
    row = dict(form="revised" if rev == "1" else "tableau", problem=kind, m=m, n=n, q=q, seed=seed, dense_cols=dense, M=model.M, N=model.N, B=B,
               slot_bytes=int(eng.slot_bytes()), pivots=int(it.sum()), passes=int(s["passes"]), rounds=int(s["lockstep_iters"]),
               ms_per_batch_median=float(np.median(ms)), ms_per_batch_min=float(np.min(ms)), reps=reps,
               max_rel_obj_diff_vs_tableau=float(np.max(np.abs(obj - ref) / (1 + np.abs(ref)))))
    print(json.dumps(row), flush=True)
    eng.close()
