#!/usr/bin/env python3
"""What do canonical optimal points cost in the dual variant?  S-small (BASELINE configs[1]) through bslv_vlp_solve_dual2 to termination
with BSLV_VLP_CANONICAL off and on, three runs each, alternating: LPs of all phases, outer iterations, points of the upper image in the
result, tie iterations per LP and wall time (phases 0 and 1 included: they are the same in both arms).  The dual driver does not report
pivots, so pivots per LP are not in the table.  No threshold is set -- profiles/canonical_obj_cost.txt holds the recorded run.

    python scripts/canonical_obj_cost.py [workload] [batch] [runs] [file to write the table to as well]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bensolve_amd import synth, vlp


def run(prob, batch, on):
    t0 = time.perf_counter()
    out = vlp.solve_primal(prob, batch=batch, alg_phase2="dual", canonical=bool(on))
    sec = time.perf_counter() - t0
    assert out["status"] == "optimal", out
    d = out["dump"]
    return dict(on=on, seconds=sec, lps=int(out["lps"]), steps=int(out["steps"]), points=int(((d["pu"] != 0) & (d["pi"] == 0)).sum()), tie=out["canonical_obj"])


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S-small"
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    prob = synth.CONFIGS[name]()
    run(prob, batch, 0)                                  # (warm-up: code objects, allocator)
    lines = ["%s through the dual variant to termination, batch %d, eps 1e-7, %d runs each, alternating" % (name, batch, runs),
             "%-4s %-6s %8s %8s %8s %10s %12s %9s" % ("run", "flag", "steps", "LPs", "points", "tie it.", "tie it./LP", "ms")]
    rows = []
    for k in range(runs):
        for on in (0, 1):
            r = run(prob, batch, on)
            rows.append(r)
            lines.append("%-4d %-6s %8d %8d %8d %10d %12.4f %9.1f" % (k, "can." if on else "off", r["steps"], r["lps"], r["points"], r["tie"]["tie_iters"],
                                                                     r["tie"]["tie_iters"] / max(1, r["lps"]), 1e3 * r["seconds"]))
    for on in (0, 1):
        sel = sorted(r["seconds"] for r in rows if r["on"] == on)
        one = [r for r in rows if r["on"] == on][0]
        lines.append("%s: median %.1f ms (min %.1f, max %.1f); %d LPs, %d points; tie phase: %s" % (
            "canonical" if on else "off      ", 1e3 * sel[len(sel) // 2], 1e3 * sel[0], 1e3 * sel[-1], one["lps"], one["points"], one["tie"]))
    text = "\n".join(lines)
    print(text, flush=True)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
