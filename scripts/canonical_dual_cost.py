#!/usr/bin/env python3
"""What do canonical duals cost (or save)?  S-small (BASELINE configs[1]) to termination with bslv_benson_set_canonical off and on,
five runs each, alternating: LPs solved, cuts applied, pivots per LP (tie pivots included, and on their own) and wall time.
Facet-defining cuts may need fewer LPs overall; no threshold is set -- profiles/canonical_dual_cost.txt holds the recorded run.

    python scripts/canonical_dual_cost.py [workload] [batch] [runs] [file to write the table to as well]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine


def run(prob, batch, on):
    eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * batch + 64)
    eng.set_canonical(on)
    t0 = time.perf_counter()
    assert eng.start() == 0
    steps = eng.run(batch)
    sec = time.perf_counter() - t0
    tot, cs = eng.totals(), eng.canonical_stats()["total"]
    eng.close()
    return dict(on=on, steps=steps, seconds=sec, lps=tot["lps"], cuts=tot["cuts"], pivots=tot["pivots"], tie=cs)


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-small"
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    prob = synth.CONFIGS[name]()
    run(prob, batch, 0)                                  # (warm-up: code objects, allocator)
    lines = ["%s to termination, batch %d, eps 1e-7, %d runs each, alternating" % (name, batch, runs),
             "%-4s %-4s %8s %8s %8s %10s %12s %10s %12s %9s" % ("run", "dual", "steps", "LPs", "cuts", "pivots", "pivots/LP", "tie piv.", "tie piv./LP", "seconds")]
    rows = []
    for k in range(runs):
        for on in (0, 1):
            r = run(prob, batch, on)
            rows.append(r)
            lines.append("%-4d %-4s %8d %8d %8d %10d %12.3f %10d %12.4f %9.3f" % (k, "can." if on else "off", r["steps"], r["lps"], r["cuts"], r["pivots"], r["pivots"] / max(1, r["lps"]),
                                                                                r["tie"]["tie_pivots"], r["tie"]["tie_pivots"] / max(1, r["lps"]), r["seconds"]))
    for on in (0, 1):
        sel = sorted(r["seconds"] for r in rows if r["on"] == on)
        one = [r for r in rows if r["on"] == on][0]
        lines.append("%s: median %.3f s (min %.3f, max %.3f); %d LPs, %d cuts, %.3f pivots per LP; tie phase: %s" % (
            "canonical" if on else "off      ", sel[len(sel) // 2], sel[0], sel[-1], one["lps"], one["cuts"], one["pivots"] / max(1, one["lps"]), one["tie"]))
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
