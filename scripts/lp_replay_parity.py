#!/usr/bin/env python3
"""What the host side of the LP engine's basis replay and tableau passes computes, as a listing that two builds can be compared by:
one line per item, a SHA-256 of the raw bytes of every array and the integer statistics verbatim.  Run it with each build's tree as
the working directory and compare the two outputs byte for byte (profiles/lp_replay_parity.txt).

The models, cases and helpers are those of tests/test_lp_refactor_gpu.py and tests/test_lp_refactor_period_gpu.py ("main" 40 x 300,
"wide" 120 x 6000 with six dense columns).  Needs a GPU.

    python scripts/lp_replay_parity.py > listing.txt
"""
import contextlib
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bensolve_amd import synth                                  # noqa: E402
from bensolve_amd.lp import LpEngine                            # noqa: E402
import test_lp_refactor_gpu as rf                               # noqa: E402
import test_lp_refactor_period_gpu as per                       # noqa: E402

INTS = ("lockstep_iters", "pivots", "passes", "launches")


def sha(a):
    a = np.ascontiguousarray(a)
    return "%s %s %s" % (a.dtype, "x".join(str(n) for n in a.shape), hashlib.sha256(a.tobytes()).hexdigest())


OUT = sys.stdout


def line(tag, what, value):
    OUT.write("%s %s: %s\n" % (tag, what, value))
    OUT.flush()


def ints(d, keys=None):
    return " ".join("%s=%d" % (k, d[k]) for k in (keys or sorted(d)))


def result(tag, res):
    for k in ("obj", "w", "y"):
        line(tag, k, sha(res[k]))


def case_a(case):
    """first generation, then refactor(dst)"""
    p = rf._problem(case)
    eng, st, it = rf._first_generation(case)
    line("a %s" % case, "status", sha(st)); line("a %s" % case, "it", sha(it))
    st2 = eng.refactor(p["dst"])
    line("a %s" % case, "refactor status", sha(np.asarray(st2)))
    line("a %s" % case, "last_refactor_stats", ints(eng.last_refactor_stats()))
    for s in p["dst"]:
        h, X = eng.get_inverse(int(s))
        line("a %s slot %d" % (case, s), "heads", sha(h)); line("a %s slot %d" % (case, s), "X", sha(X))
    result("a %s after" % case, rf._read(eng, p["model"], p["dst"]))
    eng.close()


def case_b(case, K):
    """_generations with the period K; the engine's last_stats are recorded as _generations reads them"""
    seen = []
    plain = LpEngine.last_stats

    def recording(self):
        s = plain(self)
        seen.append(s)
        return s
    LpEngine.last_stats = recording
    try:
        out = per._generations(case, K, check=False)
    finally:
        LpEngine.last_stats = plain
    assert len(seen) == 3
    for k, name in enumerate(("cold", "first", "second")):
        tag = "b %s K %d %s" % (case, K, name)
        line(tag, "it", sha(out["it"][k]))
        result(tag, out["res"][k])
        line(tag, "last_period_stats", ints(out["stats"][k]))
        line(tag, "last_stats", ints(seen[k], INTS))


def case_c(case):
    """the rescue of test_rescue_of_an_lp_the_cross_check_gives_up"""
    p = rf._problem(case)
    ref = rf._reference(case)
    b = int(np.nonzero(ref["it"] >= 4)[0][0])
    hook = "%d:%d" % (b, int(ref["it"][b]) // 2)
    eng, st, it = rf._first_generation(case, hook=hook, switch=1)
    tag = "c %s hook %s" % (case, hook)
    line(tag, "status", sha(st)); line(tag, "it", sha(it))
    line(tag, "last_refactor_stats", ints(eng.last_refactor_stats()))
    line(tag, "last_stats", ints(eng.last_stats(), INTS))
    result(tag + " first", rf._read(eng, p["model"], p["dst"]))
    second, it2 = rf._second_generation(eng, case)
    line(tag + " second", "it", sha(it2))
    result(tag + " second", second)
    eng.close()


def case_d():
    """the objective batches of test_objective_batches_with_a_period"""
    m, n, q, seed, B = 40, 300, 3, 5, 16
    rng = np.random.default_rng(seed)
    base = synth.covering_vlp(m, n, q, seed)
    prob = rf._sparse_covering(m, n, q, seed)
    mask = prob["P"] != 0
    mask[rng.integers(q, size=n), np.arange(n)] = True
    prob = dict(prob, P=base["P"] * mask)
    model = rf._P1Model(prob)
    W = rng.uniform(0.1, 1.0, size=(B, q))
    W /= W.sum(axis=1, keepdims=True)
    W2 = np.abs(W * rng.uniform(0.8, 1.2, size=W.shape))
    W2 /= W2.sum(axis=1, keepdims=True)
    for K in (0, 6):
        out, made = per._obj_run(model, prob, W, W2, K)
        line("d K %d" % K, "refactorisations", "%d" % made)
        for name in ("first", "second"):
            result("d K %d %s" % (K, name), out[name])


def case_e(case, lazy):
    """the tableau form with set_profile(1): first and second generation; with lazy tableaux the first generation is parked"""
    p = rf._problem(case)
    eng = per._engine(case, rev="0")
    eng.set_profile(1)
    tag = "e %s %s" % (case, "lazy+park" if lazy else "plain")
    per._cold(eng, case)
    line(tag + " cold", "last_stats", ints(eng.last_stats(), INTS))
    if lazy:
        eng.set_lazy(1)
    for name, run, slots in (("first", per._first, p["dst"]), ("second", per._second, p["dst2"])):
        st, it = run(eng, case)
        line(tag + " " + name, "status", sha(st)); line(tag + " " + name, "it", sha(it))
        line(tag + " " + name, "last_stats", ints(eng.last_stats(), INTS))
        result(tag + " " + name, rf._read(eng, p["model"], slots))
        if lazy:
            if name == "first":
                eng.park(slots)
            eng.discard_pending()
            line(tag + " " + name, "park_stats", ints(eng.park_stats()))
    eng.close()


def main():
    with contextlib.redirect_stdout(sys.stderr):          # (what the helpers print carries wall-clock figures: no part of the listing)
        for case in ("main", "wide"):
            case_a(case)
            for K in (6, 20):
                case_b(case, K)
            case_c(case)
        case_d()
        for case in ("main", "wide"):
            case_e(case, False)
            case_e(case, True)


if __name__ == "__main__":
    main()
