"""Probe: how far has a tableau-form slot drifted from the tableau of its basis?

A slot at generation g is the product of every rank-1 update of every ancestor back to the root; bslv_lpq_rebuild recomputes it from
the model.  The probe runs a workload with the defaults, and at the end, for every resident parent slot, reads the duals of the per-LP
rows (the cut normal w) and the objective, rebuilds the slot in place, and reads them again.  Per generation depth it prints the number
of slots and the worst relative change of the duals (max |w' - w| / (1 + max |w|)) and of the objective (|z' - z| / (1 + |z|)).
No threshold: the number is the finding.

    python scripts/probe/tableau_drift.py [--out profiles/lp_tableau_drift.txt] [--max-steps N]

Workloads: S-small to termination, and covering q=4 m=300 n=150 (seed 1) to termination or --max-steps outer iterations."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine
from bensolve_amd.lp import P2Model


def resident(eng):
    import ctypes
    cap = 1 << 16
    slots, gen = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    eng.lib.bslv_benson_resident_slots.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    n = eng.lib.bslv_benson_resident_slots(eng.h, cap, slots.ctypes.data, gen.ctypes.data)
    return slots[:n].copy(), gen[:n].copy()


def probe(name, prob, max_steps, batch=2048):
    model = P2Model(prob)
    eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * batch + 64)
    assert eng.start() == 0
    steps = eng.run(batch, max_steps)
    tot = eng.totals()
    left = eng.lib.bslv_benson_unprocessed_left(eng.h)
    slots, gen = resident(eng)
    slots = np.concatenate([[0], slots]).astype(np.int32)          # slot 0: the root tableau, one generation from the standard basis
    gen = np.concatenate([[1], gen])
    lines = ["%s: %d outer iterations (%s), %d LPs, %d cuts, %d pivots; %d resident parent slots + the root tableau" % (
        name, steps, "terminated" if left == 0 else "%d vertices left" % left, tot["lps"], tot["cuts"], tot["pivots"], len(slots) - 1)]
    w0 = eng.lp_call("dual", slots, model.var_first, model.r)
    z0 = eng.lp_call("obj", slots)
    failed = 0
    for k in range(0, len(slots), 256):
        failed += int(np.sum(eng.lp_call("rebuild", slots[k:k + 256]) != 0))
    w1 = eng.lp_call("dual", slots, model.var_first, model.r)
    z1 = eng.lp_call("obj", slots)
    eng.close()
    dw = np.max(np.abs(w1 - w0), axis=1) / (1.0 + np.max(np.abs(w0), axis=1))
    dz = np.abs(z1 - z0) / (1.0 + np.abs(z0))
    lines.append("  rebuilds that found the basis singular: %d" % failed)
    lines.append("  %10s %8s %14s %14s" % ("generation", "slots", "worst d(duals)", "worst d(obj)"))
    for g in sorted(set(gen.tolist())):
        m = gen == g
        lines.append("  %10d %8d %14.3e %14.3e" % (g, int(m.sum()), float(dw[m].max()), float(dz[m].max())))
    lines.append("  %10s %8d %14.3e %14.3e" % ("all", len(slots), float(dw.max()), float(dz.max())))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_tableau_drift.txt"))
    ap.add_argument("--max-steps", type=int, default=100000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe needs the GPU"
    out = ["Drift of tableau-form slots against a rebuild from the model (scripts/probe/tableau_drift.py; MI355X)",
           "per generation depth: resident parent slots, worst relative change of the duals of the per-LP rows and of the objective", ""]
    for name, prob in (("S-small (covering q=3 m=200 n=100)", synth.CONFIGS["S-small"]()), ("covering q=4 m=300 n=150 seed 1", synth.covering_vlp(300, 150, 4, 1))):
        lines = probe(name, prob, args.max_steps)
        print("\n".join(lines), flush=True)
        out += lines + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
