"""Cost of bslv_lpq_refactor on the two models of tests/test_lp_refactor_gpu.py: milliseconds and replay pivots per refactorised
slot (profiles/lp_refactor_cost.txt).  Usage: python scripts/lp_refactor_cost.py [repeats]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    os.environ["BSLV_LP_REV"] = "1"
    import test_lp_refactor_gpu as t
    for case in ("main", "wide"):
        p = t._problem(case)
        model = p["model"]
        eng, st, it = t._first_generation(case)
        assert np.all(st == 4)
        for slots, label in ((p["dst"][:1], "one slot"), (p["dst"], "%d slots in lock step" % p["B"])):
            eng.refactor(slots)          # (allocations, first launches)
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.refactor(slots)
                ms.append((time.perf_counter() - t0) * 1e3)
            s = eng.last_refactor_stats()
            print("case %-4s M %4d N %5d %-22s: %8.3f ms per call (median of %d), %7.3f ms and %5.1f replay pivots per slot, %d rounds of KP = 6" % (
                case, model.M, model.N, label, float(np.median(ms)), reps, float(np.median(ms)) / len(slots), s["replay_pivots"] / len(slots),
                -(-max(1, s["replay_pivots"] // len(slots)) // 6)))
        t0 = time.perf_counter()
        eng.solve_batch(p["dst"], p["dst2"], np.full((p["B"], model.r), -np.inf), p["ub2"])
        print("case %-4s for scale: the second-generation batch of %d LPs: %.3f ms, %d pivots" % (case, p["B"], (time.perf_counter() - t0) * 1e3, eng.last_stats()["pivots"]))
        eng.close()


if __name__ == "__main__":
    main()
