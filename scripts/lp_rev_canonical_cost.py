"""What canonical duals cost in the REVISED LP form (bslv_lpq_solve_batch_canonical, the tie phase k_select_tie_rev), in one process:

  S-mid   the bench's S-mid problem through the Benson driver on a revised LP engine, batches of 64 P2(v) LPs: the first `batches`
          outer iterations, once with bslv_benson_set_canonical off (the driver calls solve_batch) and once with it on (it calls
          bslv_lpq_solve_batch_canonical).  Per batch: the time of solve_local between two HIP events -- the call is stream-synchronised,
          so the events bracket the LP work of the batch and the read-back of its duals -- LPs, pivots and tie pivots.
  ex09    tests/golden/ex/ex09.vlp, all phases by the command-line driver with BSLV_LP_REV=1, without and with BSLV_CANONICAL_DUAL=1,
          under BSLV_LP_TIMING=1: the library's own line per solve_batch call (host clock around the synchronised call) gives the
          first phase-2 batches, the line of the tie phase their tie pivots; LPs, seconds and tie pivots of the whole runs.
          (opt-in: about two minutes of GPU time)

One JSON line per case.
usage: lp_rev_canonical_cost.py [S-mid|ex09|both] [batches]"""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def smid(batches, batch=64):
    import ctypes
    import torch
    os.environ["BSLV_LP_REV"] = "1"          # read at create
    from bensolve_amd import synth
    from bensolve_amd.benson import BensonEngine
    prob = synth.CONFIGS["S-mid"]()
    out = dict(case="S-mid through the Benson driver, revised LP form, batches of %d" % batch, batches=batches)
    for arm, on in (("solve_batch", 0), ("solve_batch_canonical", 1)):
        eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * batch + 64)
        eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
        assert eng.lib.bslv_lpq_is_revised(eng._lp_h) == 1
        eng.set_canonical(on)
        assert eng.start() == 0
        rows = []
        for _ in range(batches):
            nl, nt = eng.collect(batch)
            if nt == 0:
                break
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rec, piv, ls = eng.solve_local(nl)
            e1.record()
            e1.synchronize()
            cs = eng.canonical_stats()["last"]
            rows.append(dict(lps=nl, ms=round(e0.elapsed_time(e1), 3), pivots=int(piv), tie_pivots=cs["tie_pivots"], entered=cs["entered"], gave_up=cs["capped"],
                             optimal=int((rec[:, 1] == 4).sum())))
            eng.apply(rec)
        eng.close()
        full = [r for r in rows[1:] if r["lps"] == batch] or rows      # (the first batch holds the few vertices of the start)
        lps = sum(r["lps"] for r in full)
        out[arm] = dict(batches=rows, full_batches=len(full), ms_median=float(np.median([r["ms"] for r in full])), ms_min=min(r["ms"] for r in full), ms_max=max(r["ms"] for r in full),
                        pivots_per_lp=sum(r["pivots"] for r in full) / lps, tie_pivots_per_lp=sum(r["tie_pivots"] for r in full) / lps)
    print(json.dumps(out), flush=True)


def ex09(batches):
    cli = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
    vlp = os.path.join(ROOT, "tests", "golden", "ex", "ex09.vlp")
    out = dict(case="ex09 all phases, command-line driver, revised LP form, -e 1e-2", first_batches=batches)
    tmp = tempfile.mkdtemp()
    for arm, on in (("off", None), ("canonical", "1")):
        env = dict(os.environ, BSLV_LP_REV="1", BSLV_LP_TIMING="1")
        env.pop("BSLV_CANONICAL_DUAL", None)
        if on:
            env["BSLV_CANONICAL_DUAL"] = on
        base = os.path.join(tmp, "ex09_cost_%s" % arm)
        t0 = time.perf_counter()
        p = subprocess.run([cli, vlp, "-e", "1e-2", "-o", base], env=env, capture_output=True, text=True, timeout=900)
        secs = time.perf_counter() - t0
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        calls = []
        for line in p.stderr.splitlines():
            m = re.match(r"lp solve_batch: revised form (\d+) x (\d+), B (\d+), (\d+) lock-step rounds, (\d+) pivots, (\d+) passes, ([0-9.]+) ms", line)
            if m:
                calls.append(dict(B=int(m.group(3)), rounds=int(m.group(4)), pivots=int(m.group(5)), ms=float(m.group(7)), tie_pivots=0, entered=0, gave_up=0))
            m = re.match(r"lp tie phase[^:]*: (\d+) LPs entered, (\d+) tie pivots, (\d+) without an entering candidate, (\d+) gave up", line)
            if m and calls:
                calls[-1].update(entered=int(m.group(1)), tie_pivots=int(m.group(2)), gave_up=int(m.group(4)))
        m = re.search(r"Number of LPs solved: (\d+)", p.stdout)
        # phase 2's batches: the calls of more than one LP (phases 0 and 1 and the retries of single LPs solve one at a time)
        multi = [c for c in calls if c["B"] > 1]
        out[arm] = dict(seconds=round(secs, 1), lps_reported=int(m.group(1)) if m else None, solve_calls=len(calls), lps_in_calls=sum(c["B"] for c in calls),
                        pivots=sum(c["pivots"] for c in calls), tie_pivots=sum(c["tie_pivots"] for c in calls), entered=sum(c["entered"] for c in calls),
                        gave_up=sum(c["gave_up"] for c in calls), first_batches=multi[:batches], stdout_tail=p.stdout.strip().splitlines()[-6:])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "S-mid"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    if what in ("S-mid", "both"):
        smid(n)
    if what in ("ex09", "both"):
        ex09(n)
