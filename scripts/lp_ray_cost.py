"""HIP-event time of k_ray and of bslv_lpq_certify_rays on a batch of 2048 LPs (profiles/lp_ray_cost.txt).

    BSLV_LP_RAY_TIMING=1 BSLV_LP_CERTIFY_TIMING=1 python scripts/lp_ray_cost.py [M N]

The batch: the 16 LPs of tests/lp_ray_cases.py: boxed_set(M, N) 128 times over (384 INFEASIBLE LPs with a Farkas vector, 1664 OPTIMAL
ones), solved from one parent slot in both forms; the engine prints the times on stderr, this script the statuses and verdicts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lp_ray_cases as rc
from bensolve_amd.lp import LpEngine


def main():
    M, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (33, 257)
    s = rc.boxed_set(M, N)
    B = 2048
    vlo, vup = np.tile(s["vlo"], (B // rc.NLP, 1)), np.tile(s["vup"], (B // rc.NLP, 1))
    for form in ("tableau", "revised"):
        if form == "revised":
            os.environ["BSLV_LP_REV"] = "1"
        else:
            os.environ.pop("BSLV_LP_REV", None)
        eng = LpEngine(M, N, s["A"], s["lo"], s["up"], s["cost"], 0, M, 1 + B)
        assert eng.set_rays(1) == 0
        eng.reset_slot(0)
        eng.solve_batch([0], [0], vlo[:1], vup[:1])
        dst = np.arange(1, 1 + B, dtype=np.int32)
        for rep in range(3):
            st, it = eng.solve_batch(np.zeros(B, np.int32), dst, vlo, vup)
            out = eng.certify_rays(dst, vlo, vup)
            print("lp_ray_cost %s %d x %d rep %d: %d LPs, %d INFEASIBLE, rays %s, total_ms of the solve %.3f, verdict 0 for %d, kind NONE for %d" % (
                form, M, N, rep, B, int(np.sum(st == 0)), eng.last_ray_stats(), eng.last_stats()["total_ms"], int(np.sum(out["verdict"] == 0)), int(np.sum(out["verdict"] & 8 != 0))), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
