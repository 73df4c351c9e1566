#!/usr/bin/env python3
"""What does a compaction of the resident polyhedron cost and free at S-mid's size?  (bslv_poly_compact)

Runs S-mid as bench.py does -- the ramp to one full batch, 4 untimed and 20 timed steps of 2048 LPs -- three times: with the driver's
trigger off, with f = 0.5 and with f = 0.25, both at the default min_slots (65536), and writes profiles/poly_compact_smid.txt:

    python scripts/poly_compact_probe.py [--out FILE] [--steps 20] [--warmup 4] [--batch 2048] [--workload S-mid]
    python scripts/poly_compact_probe.py --per-step --workload S-degenerate --batch 64 --steps 9 --out FILE
        # slots and pool words after every step, trigger off and f = 0.5: which 32-bit limit the run meets first

Per run: steps/s and LPs/s over the timed window, the final slots / live elements / pool words used / pool words of live lists / bytes
(bslv_poly_garbage).  Per compaction: slots and pool words before -> after, the microseconds of the call (host clock around it:
allocation, kernels, the synchronisations and the frees), and the bytes it had to move per microsecond -- read + write of the
coordinates, flag, class and length of every live element, of the live pool words and of the edge list -- beside the memory rate of
the card (HBM3E: 8.0 TB/s by specification, about 6.3 TB/s reached by a plain copy kernel = 8.0 / 6.3 MB per microsecond).
None of the figures is a gate: the switch ships off."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine


def one_run(prob, f, args, log):
    import torch
    B = args.batch
    q = prob["q"]
    eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * B + 64)
    if f > 0:
        eng.set_compact(f, -1)
    assert eng.start() == 0
    events = []
    seen = [0]

    def step(tag):
        s = eng.step(B)
        st = eng.poly_call("last_compact_stats")
        if st["calls"] > seen[0]:
            seen[0] = st["calls"]
            g = eng.poly_call("garbage")                 # (after the call: slots = live, pool used = pool live)
            moved = 2 * (g["live"] * (8 * q + 1 + 1 + 4) + 4 * g["pool_live"] + 8 * g["edges"])
            events.append((tag, g["slots"] + st["slots_removed"], g["slots"], g["pool_used"] + st["pool_removed"], g["pool_used"], st["us"], moved, st["bytes_returned"]))
        return s
    ramp = 0
    while True:
        s = step("ramp %d" % ramp)
        ramp += 1
        if eng.poly_call("unprocessed", 0)[3] >= B or ramp > 200 or s["lps"] == 0:
            break
    for k in range(args.warmup):
        step("warm-up %d" % k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lps = 0
    for k in range(args.steps):
        lps += step("timed %d" % k)["lps"]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    g = eng.poly_call("garbage")
    cs = eng.compact_stats()
    tot = eng.totals()
    eng.close()
    log("run: trigger %s" % ("off" if f == 0 else "f = %g, min_slots = 65536 (default)" % f))
    log("  ramp %d steps, then %d untimed + %d timed steps of %d" % (ramp, args.warmup, args.steps, B))
    log("  window: %.3f s, %.2f steps/s, %.1f k LPs/s" % (dt, args.steps / dt, lps / dt / 1e3))
    log("  totals of the run: %d LPs, %d cuts, %d pivots" % (tot["lps"], tot["cuts"], tot["pivots"]))
    log("  final: %d slots, %d live, %d pool words used, %d pool words of live lists, %d edges, %.1f MB of element / pool / edge arrays" % (
        g["slots"], g["live"], g["pool_used"], g["pool_live"], g["edges"], g["bytes"] / 1e6))
    log("  compactions: %d, %d slots and %d pool words removed, %.2f ms in all" % (cs["compactions"], cs["slots_removed"], cs["pool_removed"], cs["us"] / 1e3))
    for tag, s0, s1, p0, p1, us, moved, back in events:
        log("    after step '%s': slots %d -> %d, pool words %d -> %d, %d us, %.1f MB moved = %.3f MB/us (HBM: 8.0 by specification, 6.3 by a copy kernel), %.1f MB handed back" % (
            tag, s0, s1, p0, p1, us, moved / 1e6, moved / 1e6 / max(us, 1), back / 1e6))
    log("")
    return dict(f=f, lps_per_sec=lps / dt, totals=tot)


def per_step_run(prob, f, args, log, keep_cap=False):
    """--per-step: slots and pool words after every step, for the question which 32-bit limit a long run meets first
    (2^30 elements, 2^30 edges, 0xF0000000 pool words) and how far compaction moves it"""
    from bensolve_amd._lib import BslvError
    B = args.batch
    eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * B + 64)
    if f > 0:
        eng.set_compact(f, -1)
    if keep_cap:
        eng.poly_call("debug_set", 21, 1)
    assert eng.start() == 0
    log("run: trigger %s%s, steps of %d" % ("off" if f == 0 else "f = %g, min_slots = 65536 (default)" % f,
                                            ", the compactions keep the old capacities (test hook: bslv_poly_debug_set key 21)" if keep_cap else "", B))
    log("  step: seconds | slots, live, pool words used, pool words of live lists, edges, MB | compactions so far")
    k = 0
    try:
        while k < args.steps:
            t0 = time.perf_counter()
            s = eng.step(B)
            dt = time.perf_counter() - t0
            g = eng.poly_call("garbage")
            k += 1
            r2, tot = eng.poly_call("rounds2_stats"), eng.totals()
            log("  %3d: %7.2f s | %d, %d, %d, %d, %d, %.0f | %d | LPs %d, cuts %d, pivots %d; rounds %d with %d cuts, %d taken back for want of capacity" % (
                k, dt, g["slots"], g["live"], g["pool_used"], g["pool_live"], g["edges"], g["bytes"] / 1e6, eng.compact_stats()["compactions"],
                tot["lps"], tot["cuts"], tot["pivots"], r2["rounds"], r2["cuts"], r2["declined"]))
            if args.check:
                ck = eng.poly_call("check", 0, (0, min(256, g["live"])))
                log("       bslv_poly_check, pairs of the first 256 rows: %s %s" % ("clean" if ck["clean"] else "NOT CLEAN", ck["out"]))
            if s["lps"] == 0 and s["left"] == 0:
                break
    except BslvError as e:
        log("  stopped in step %d: %s" % (k + 1, e))
    cs = eng.compact_stats()
    log("  compactions: %d, %d slots and %d pool words removed, %.1f ms in all" % (cs["compactions"], cs["slots_removed"], cs["pool_removed"], cs["us"] / 1e3))
    log("")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-step", action="store_true", help="slots and pool words after each of --steps steps (no ramp, no warm-up), trigger off and f = 0.5")
    ap.add_argument("--keep-cap", action="store_true", help="--per-step: a third run, f = 0.5 with compactions that keep the old capacities -- renumbering and packing alone")
    ap.add_argument("--check", action="store_true", help="--per-step: bslv_poly_check after every step (incidences, edges and halfspaces of the whole polyhedron, pairs of its first 256 rows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_compact_smid.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--workload", default="S-mid")
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.per_step:                       # (a long run: what is known so far survives a time limit)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log("# python scripts/poly_compact_probe.py --workload %s --batch %d --warmup %d --steps %d" % (args.workload, args.batch, args.warmup, args.steps))
    log("# bslv_poly_compact through the Benson driver's trigger (bslv_benson_set_compact); host clocks; one process, the runs one after the other")
    log("")
    prob = synth.CONFIGS[args.workload]()
    if args.per_step:
        lines[0] += " --per-step"
        for f in (0.0, 0.5):
            per_step_run(prob, f, args, log)
        if args.keep_cap:
            per_step_run(prob, 0.5, args, log, keep_cap=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    rows = [one_run(prob, f, args, log) for f in (0.0, 0.5, 0.25)]
    same = all(r["totals"] == rows[0]["totals"] for r in rows)
    log("LPs, cuts and pivots of the three runs are %s" % ("identical: the trajectory does not depend on the names of the elements" if same else "NOT identical"))
    log("LPs/s against the run with the trigger off: " + ", ".join("f = %g: %+.1f %%" % (r["f"], 100 * (r["lps_per_sec"] / rows[0]["lps_per_sec"] - 1)) for r in rows[1:]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
