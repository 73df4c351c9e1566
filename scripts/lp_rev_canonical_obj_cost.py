"""What canonical optimal points cost in the REVISED LP form (bslv_lpq_solve_batch_obj_canonical, the tie phase k_select_tie_obj_rev):

  S-mid   P1(w) of the bench's S-mid problem (tests' P1Model restated: rows [A 0; -P I], the weights as the costs of the q columns y)
          on two revised LP engines in one process: the feasibility LP and PART 1's solve in slot 0, then `batches` batches of 64
          weights from slot 0 -- half of each batch generic (uniform on the simplex), half with one or two zero entries (normals of
          unbounded faces of the upper image: dual degenerate LPs) -- once by solve_batch_obj and once by the new call.  Per batch: the
          host clock around the call (it is stream-synchronised and reads status and iterations back), pivots, tie iterations.
  ex09    tests/golden/ex/ex09.vlp, all phases by the command-line driver with -a dual -e 1e-2 and BSLV_LP_REV=1, without and with
          BSLV_CANONICAL_OBJ_CALL=1, under BSLV_LP_TIMING=1: the library's own line per objective batch and the line of its tie
          phase; LPs, seconds and tie iterations of the whole runs.  (opt-in: minutes of GPU time; a time limit per arm, and an arm
          that does not end within it is reported as such)

One JSON line per case.
usage: lp_rev_canonical_obj_cost.py [S-mid|<another name of synth.CONFIGS>|ex09|both] [batches] [ex09 seconds per arm]"""
import ctypes
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


def p1_engine(prob, slots):
    from bensolve_amd.lp import LpEngine, bounds_from_types
    m, n, q = prob["m"], prob["n"], prob["q"]
    M, N = m + q, n + q
    L = np.zeros((M, N))
    L[:m, :n] = prob["A"]
    L[m:, :n] = -prob["P"]
    L[m:, n:] = np.eye(q)
    rlo, rup = bounds_from_types(prob["rtype"], prob["rlb"], prob["rub"])
    clo, cup = bounds_from_types(prob["ctype"], prob["clb"], prob["cub"])
    lo = np.concatenate([rlo, np.zeros(q), clo, np.full(q, -np.inf)])
    up = np.concatenate([rup, np.zeros(q), cup, np.full(q, np.inf)])
    eng = LpEngine(M, N, L, lo, up, np.zeros(N + 1), 0, 0, slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
    return eng, M + n


def weights(q, batch, rng):
    W = rng.dirichlet(np.ones(q), size=batch)
    for b in range(batch // 2, batch):
        W[b, rng.choice(q, size=1 + b % 2, replace=False)] = 0.0
    return W / W.sum(axis=1, keepdims=True)


def smid(batches, batch=64, config="S-mid"):
    os.environ["BSLV_LP_REV"] = "1"          # read at create
    from bensolve_amd import synth
    prob = synth.CONFIGS[config]()
    q = prob["q"]
    ddir = 1.0 + np.array([synth_hash(k) for k in range(q)])
    rng = np.random.default_rng(3)
    Ws = [weights(q, batch, rng) for _ in range(batches)]
    out = dict(case="%s P1(w), revised LP form, batches of %d from slot 0" % (config, batch), batches=batches)
    for arm in ("solve_batch_obj", "solve_batch_obj_canonical"):
        eng, y_first = p1_engine(prob, batch + 1)
        assert eng.set_refactor(1) == 0      # (the cold feasibility LP of this model drifts past the pivot cross-check: the in-call rescue, in both arms)
        eng.reset_slot(0)
        st, it0 = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
        if st[0] != 4:                       # (no start, no batches: reported, not worked around)
            out[arm] = dict(start="the cold feasibility LP came back with status %d after %d iterations" % (int(st[0]), int(it0[0])))
            eng.close()
            continue
        st, _ = eng.solve_batch_obj([0], [0], y_first, np.full((1, q), 1.0 / q))
        assert st[0] == 4, st
        src, dst = np.zeros(batch, np.int32), np.arange(1, batch + 1, dtype=np.int32)
        rows = []
        for W in Ws:
            t0 = time.perf_counter()
            if arm == "solve_batch_obj":
                st, it = eng.solve_batch_obj(src, dst, y_first, W)
            else:
                st, it = eng.solve_batch_obj_canonical(ddir, src, dst, y_first, W)
            ms = 1e3 * (time.perf_counter() - t0)
            cs = eng.last_canonical_obj_stats()
            rows.append(dict(lps=batch, ms=round(ms, 3), iters=int(it.sum()), optimal=int((st == 4).sum()), entered=cs["entered"], tie_iters=cs["tie_iters"],
                             unbounded=cs["unbounded"], gave_up=cs["capped"]))
        eng.close()
        out[arm] = dict(batches=rows, ms_median=float(np.median([r["ms"] for r in rows])), ms_min=min(r["ms"] for r in rows), ms_max=max(r["ms"] for r in rows),
                        iters_per_lp=sum(r["iters"] for r in rows) / (batch * len(rows)), tie_iters_per_lp=sum(r["tie_iters"] for r in rows) / (batch * len(rows)))
    print(json.dumps(out), flush=True)


def synth_configs():
    from bensolve_amd import synth
    return synth.CONFIGS


def synth_hash(k):
    """hash01 of bensolve_amd/csrc/common.h, as tests/canonical_cases.direction restates it: the driver's direction is 1 + hash01(k)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import canonical_cases as cc
    return float(cc.direction(k + 1)[k] - 1.0)


def ex09(batches, limit):
    cli = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
    vlp = os.path.join(ROOT, "tests", "golden", "ex", "ex09.vlp")
    out = dict(case="ex09 all phases, command-line driver, revised LP form, -a dual -e 1e-2", first_batches=batches, seconds_per_arm=limit)
    tmp = tempfile.mkdtemp()
    for arm, on in (("off", None), ("canonical_call", "1")):
        env = dict(os.environ, BSLV_LP_REV="1", BSLV_LP_TIMING="1")
        env.pop("BSLV_CANONICAL_OBJ", None)
        env.pop("BSLV_CANONICAL_OBJ_CALL", None)
        if on:
            env["BSLV_CANONICAL_OBJ_CALL"] = on
        base = os.path.join(tmp, "ex09_obj_cost_%s" % arm)
        t0 = time.perf_counter()
        try:
            p = subprocess.run([cli, vlp, "-a", "dual", "-e", "1e-2", "-o", base], env=env, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[arm] = dict(ended=False, seconds=limit)
            print(json.dumps(out), flush=True)
            return                             # (nothing more on the GPU after a step that ran into its limit)
        secs = time.perf_counter() - t0
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        calls = []
        for line in p.stderr.splitlines():
            m = re.match(r"lp solve_batch: revised form (\d+) x (\d+), B (\d+), (\d+) lock-step rounds, (\d+) pivots, (\d+) passes, ([0-9.]+) ms", line)
            if m:
                calls.append(dict(B=int(m.group(3)), rounds=int(m.group(4)), pivots=int(m.group(5)), ms=float(m.group(7)), tie_iters=0, entered=0, gave_up=0))
            m = re.match(r"lp tie phase of an objective batch \(per call\): (\d+) LPs entered, (\d+) tie iterations, (\d+) on a column without a blocking row, (\d+) gave up", line)
            if m and calls:
                calls[-1].update(entered=int(m.group(1)), tie_iters=int(m.group(2)), gave_up=int(m.group(4)))
        m = re.search(r"Number of LPs solved: (\d+)", p.stdout)
        multi = [c for c in calls if c["B"] > 1]
        out[arm] = dict(ended=True, seconds=round(secs, 1), lps_reported=int(m.group(1)) if m else None, solve_calls=len(calls), lps_in_calls=sum(c["B"] for c in calls),
                        pivots=sum(c["pivots"] for c in calls), tie_iters=sum(c["tie_iters"] for c in calls), entered=sum(c["entered"] for c in calls),
                        gave_up=sum(c["gave_up"] for c in calls), first_batches=multi[:batches], stdout_tail=p.stdout.strip().splitlines()[-6:])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "S-mid"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    limit = int(sys.argv[3]) if len(sys.argv) > 3 else 240
    if what in synth_configs():
        smid(n, config=what)
    if what == "both":
        smid(n)
    if what in ("ex09", "both"):
        ex09(n, limit)
