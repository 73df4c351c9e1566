"""Probe: what bslv_lpq_rebuild costs in the tableau form, beside a plain pass of the tableau-update kernel over the same slots.

    BSLV_LP_BASIS_TIMING=1 python scripts/probe/lp_basis_cost.py

Two shapes: S-mid's P2 model (1011 x 506) with the bases of B LPs solved from the root tableau, and lp_cases.random_lp at (24, 1540)
with the optimal basis of its own LP.  For each: one call over B slots and one call over a single slot.  The library prints, per call,
the HIP-event time of the whole replay, of its passes and of the refresh pass alone (a plain pass: nothing pending, every row read,
written and multiplied with x_N); this script adds the slots, the replay pivots and the passes per slot from
bslv_lpq_last_rebuild_stats.  Reported only: no target is set."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ.setdefault("BSLV_LP_BASIS_TIMING", "1")
os.environ["BSLV_LP_REV"] = "0"

from bensolve_amd import synth
from bensolve_amd.lp import LpEngine, P2Model


def report(tag, eng, slots):
    for rep in range(2):                     # (the first call of a shape loads code objects and sizes the buffers)
        t = time.perf_counter()
        st = eng.rebuild(slots)
        dt = (time.perf_counter() - t) * 1e3
    s = eng.last_rebuild_stats()
    sys.stderr.flush()
    print("%s: %d slots, %d failed, %d replay pivots (%.1f per slot), %d passes (%.2f per slot), host clock of the second call %.3f ms = %.4f ms per slot" % (
        tag, len(slots), int(np.sum(st != 0)), s["replay_pivots"], s["replay_pivots"] / len(slots), s["passes"], s["passes"] / len(slots), dt, dt / len(slots)), flush=True)


def main():
    import torch
    assert torch.cuda.is_available(), "the probe needs the GPU"
    B = 64
    prob = synth.CONFIGS["S-mid"]()
    model = P2Model(prob)
    rng = np.random.default_rng(4)
    n = prob["n"]
    X = rng.random((B, n)) * (3.0 / n) + 1.0 / n
    V = (X @ prob["P"].T) * rng.uniform(0.2, 1.2, size=(B, 1)) + rng.normal(scale=0.05, size=(B, prob["q"]))
    eng = LpEngine.from_model(model, pool_slots=B + 2)
    eng.reset_slot(0)
    st, it0 = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), model.ub_for(V[:1]))
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.full((B, model.r), -np.inf), model.ub_for(V))
    print("S-mid P2 model: M %d N %d, slot %d bytes, root LP %d pivots, %d LPs from it: statuses %s, %d pivots" % (
        model.M, model.N, eng.slot_bytes(), int(it0[0]), B, sorted(set(st.tolist())), int(it.sum())), flush=True)
    report("S-mid shape, one call", eng, dst)
    report("S-mid shape, a single slot", eng, dst[:1])
    eng.close()

    import lp_cases as lc
    A, lo, up, cost = lc.random_lp(24, 1540, np.random.default_rng(2064), "feasible", bounded=True)
    eng = LpEngine(24, 1540, A, lo, up, cost, 0, 0, B + 2)
    eng.reset_slot(0)
    st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.zeros((B, 0)), np.zeros((B, 0)))
    print("(24, 1540): slot %d bytes, its own LP from the standard basis into %d slots: statuses %s, %d pivots each" % (
        eng.slot_bytes(), B, sorted(set(st.tolist())), int(it[0])), flush=True)
    report("(24, 1540), one call", eng, dst)
    report("(24, 1540), a single slot", eng, dst[:1])
    eng.close()


if __name__ == "__main__":
    main()
