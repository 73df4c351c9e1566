"""Every last_* counter getter of LpEngine after each call of a fixed sequence, on the "main" case of tests/test_lp_refactor_gpu.py
(profiles/lp_call_counters_*.txt): what a call leaves in the counters, and what a call that does nothing (B = 0) or is refused
(BSLV_E_ARG) leaves standing of the call before it.  Two builds of the library compute the same when their outputs agree in every
field but update_ms and total_ms.  Usage: python scripts/lp_call_counters.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GETTERS = ("last_stats", "last_refactor_stats", "last_period_stats", "last_pricing_stats", "last_primal_pricing_stats", "last_canonical_stats",
           "last_canonical_obj_stats", "last_ray_stats", "last_ray_certify_stats", "last_certify_stats", "last_rebuild_stats")


def show(eng, what):
    print("== " + what)
    for g in GETTERS:
        d = getattr(eng, g)()
        ms = {k: v for k, v in d.items() if k.endswith("_ms")}
        line = " ".join("%s=%d" % (k, v) for k, v in d.items() if k not in ms)
        print("   %-26s %s%s" % (g, line, "".join("  [%s %.3f]" % kv for kv in ms.items())))


def nothing_and_refused(eng, vcnt):
    """a batch of no LPs, and a batch whose dst slot lies outside the pool"""
    from bensolve_amd._lib import BslvError
    none = np.zeros(0, np.int32)
    st, _ = eng.solve_batch(none, none, np.zeros((0, vcnt)), np.zeros((0, vcnt)))
    show(eng, "a call with B = 0 (statuses: %d)" % len(st))
    try:
        eng.solve_batch([0], [eng.pool_slots], np.zeros((1, vcnt)), np.zeros((1, vcnt)))
        print("the call with a slot outside the pool was accepted")
    except BslvError as e:
        show(eng, "a refused call (%s)" % str(e).split(":")[0])


def main():
    import canonical_cases as cc
    import test_lp_refactor_gpu as t
    from bensolve_amd.lp import LpEngine
    case = "main"
    p = t._problem(case)
    model, B = p["model"], p["B"]
    lo = np.full((B, model.r), -np.inf)
    warm = lambda eng: eng.solve_batch(np.zeros(B, np.int32), p["dst"], lo, p["ub"])

    def start(rev):
        with t._env(BSLV_LP_REV=rev, BSLV_LP_REFACTOR=None, BSLV_LP_REV_DRIFT=None):
            eng = LpEngine.from_model(model, pool_slots=2 * B + 4)
        eng.reset_slot(0)
        eng.solve_batch([0], [0], lo[:1], p["ub"][:1])
        return eng

    # the revised form: cold solve, warm batch, the warm batch with a rescue, a second generation under a period
    eng = start("1")
    show(eng, "revised form: the cold solve")
    st, it = warm(eng)
    show(eng, "revised form: the warm batch of %d LPs (statuses %s)" % (B, sorted(set(st.tolist()))))
    b = int(np.nonzero(it >= 4)[0][0])
    hook = "%d:%d" % (b, int(it[b]) // 2)
    assert eng.set_refactor(1) == 0
    with t._env(BSLV_LP_REV_DRIFT=hook):
        st, _ = warm(eng)
    show(eng, "revised form: the warm batch again with set_refactor(1) and BSLV_LP_REV_DRIFT=%s (statuses %s)" % (hook, sorted(set(st.tolist()))))
    assert eng.set_refactor_period(4) == 0
    st, _ = eng.solve_batch(p["dst"], p["dst2"], lo, p["ub2"])
    show(eng, "revised form: the second generation under set_refactor_period(4) (statuses %s)" % sorted(set(st.tolist())))
    nothing_and_refused(eng, model.r)
    eng.close()
    # the tableau form with the canonical basis
    eng = start("0")
    assert eng.set_canonical(1, np.ones(model.r)) == 0
    st, _ = warm(eng)
    show(eng, "tableau form: the warm batch with set_canonical(1, ones) (statuses %s)" % sorted(set(st.tolist())))
    nothing_and_refused(eng, model.r)
    eng.close()
    # the tableau form, objective batches with the canonical point (the P1(w) model of the same problem), then a solve_batch behind it
    pm, W = t._obj_batch()
    with t._env(BSLV_LP_REV="0"):
        eng = LpEngine(pm.M, pm.N, pm.L, pm.lo, pm.up, np.zeros(pm.N + 1), 0, 0, len(W) + 2)
    eng.reset_slot(0)
    eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
    eng.solve_batch_obj([0], [0], pm.y_first, np.full((1, pm.q), 1.0 / pm.q))
    assert eng.set_canonical_obj(1, pm.y_first, cc.direction(pm.q)) == 0
    dst = np.arange(1, len(W) + 1, dtype=np.int32)
    st, _ = eng.solve_batch_obj(np.zeros(len(W), np.int32), dst, pm.y_first, W)
    show(eng, "tableau form: an objective batch of %d LPs with set_canonical_obj (statuses %s)" % (len(W), sorted(set(st.tolist()))))
    st, _ = eng.solve_batch(dst[:1], dst[:1], np.zeros((1, 0)), np.zeros((1, 0)))
    show(eng, "tableau form: a solve_batch of one of its slots onto itself (statuses %s)" % sorted(set(st.tolist())))
    nothing_and_refused(eng, 0)
    eng.close()


if __name__ == "__main__":
    main()
