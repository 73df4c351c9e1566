"""What bslv_poly_check costs (profiles/poly_check_cost.txt).
1. One full check of the polyhedron of SURVEY 8c's size (tests/golden/poly_ref_large.npz, tangent_q5_N1000: 27 418 elements) per
   kernel via HIP events (BSLV_POLY_CHECK_TIMING=1: the library prints them), wall clock of the whole call, and beside it
   bslv_poly_dual_adjacency on the same polyhedron, the existing all-pairs kernel.
2. S-small to termination with BSLV_POLY_CHECK=1 (an audit after every outer iteration) and without.
usage: poly_check_cost.py [repeats]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BSLV_POLY_CHECK_TIMING"] = "1"
import numpy as np
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine
from bensolve_amd.poly import PolyEngine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
G = np.load(os.path.join(ROOT, "tests", "golden", "poly_ref_large.npz"))
name = "tangent_q5_N1000"
q, v2h, apex, init_after = [int(x) for x in G[name + "/in_meta"]]
vals = G[name + "/in_vals"]
E = PolyEngine(q, v2h)
for k in range(init_after):
    E.add(vals[k])
assert E.init() == 0
E.add_cuts(vals[init_after:])
print("1. %s: one full bslv_poly_check (the library's own line per call follows on stderr), %d repeats" % (name, reps))
for r in range(reps):
    t0 = time.perf_counter()
    res = E.check()
    t_check = time.perf_counter() - t0
    print("   check %d: %.1f ms wall; counts %s; worst %s" % (r, t_check * 1e3, res["out"], res["worst"]), flush=True)
    assert res["clean"] and res["out"][9] == res["out"][6], res
for r in range(reps):
    t0 = time.perf_counter()
    E.dual_adjacency()
    t_da = time.perf_counter() - t0
    print("   bslv_poly_dual_adjacency %d: %.1f ms wall (%d live facets, %d dual edges)" % (r, t_da * 1e3, res["out"][1], E.lib.bslv_poly_ndual_edges(E.h)), flush=True)
for rows in ((0, 1000), (13000, 1000)):
    t0 = time.perf_counter()
    part = E.check(rows=rows)
    print("   rows %s: %.1f ms wall; [9..11] = %s" % (rows, (time.perf_counter() - t0) * 1e3, part["out"][9:]), flush=True)
E.close()

print("2. S-small to termination (batch 2048, eps 1e-7), BSLV_POLY_CHECK off / on, alternating")
del os.environ["BSLV_POLY_CHECK_TIMING"]
for r in range(reps):
    for on in (0, 1):
        os.environ["BSLV_POLY_CHECK"] = str(on)
        eng = BensonEngine(synth.CONFIGS["S-small"](), eps=1e-7, pool_slots=8192)
        t0 = time.perf_counter()
        assert eng.start() == 0
        steps = 0
        while True:
            s = eng.step(2048); steps += 1
            if s["lps"] == 0 and s["left"] == 0:
                break
        sec = time.perf_counter() - t0
        tot = eng.totals()
        print("   run %d check %s: %d outer iterations, %d LPs, %d cuts, %.3f s" % (r, "on " if on else "off", steps, tot["lps"], tot["cuts"], sec), flush=True)
        eng.close()          # (with the check on the driver's tally goes to stderr here)
