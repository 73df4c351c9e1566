"""A round's new vertices are classified by workgroups of the launch that runs its prunes (k_r2_prune_classify, the default) instead
of a launch of their own (BSLV_R2_RIDE=0: k_r2_classify3, then k2_fused_t<true>).  The classification computes the same words either
way, so both positions of the switch must build the SAME polyhedron bit for bit -- slots, coordinates, incidence lists, edges, dual
adjacency, return codes -- in every arm of the rounds, at the shape edges of the classification in the workgroups of that launch, with
the classifying workgroups capped at one (the stride over the new vertices), and on Benson steps of the bench workload."""
import os
import functools
import numpy as np
import pytest

import poly_harness as ph
from poly_harness import truncated_simplex
from bensolve_amd.poly import PolyEngine
from test_poly_modes_gpu import hooks, R2_MODES, _r2_cases

pytestmark = pytest.mark.gpu

RIDE_VARS = ("BSLV_R2_RIDE", "BSLV_R2_RIDE_G", "BSLV_R2_RIDE_T")
DUMP_KEYS = ("pu", "pi", "ps", "X", "du", "di", "Y", "E", "I", "DE")
ALWAYS = {"BSLV_R2_MIN_CUTS": "-1"}            # rounds to the end of every chunk
assert R2_MODES["rounds always"] == ALWAYS

# the arms of the rounds, each run with both positions of the switch
ARMS = {
    "default": dict(ALWAYS),
    "local minima (packed = 0)": dict(ALWAYS, BSLV_R2_MIS="0"),
    "nothing queued ahead": dict(ALWAYS, BSLV_R2_SPEC="0"),
    "chunks of 96, declined rounds": dict(ALWAYS, BSLV_CHUNK_CUTS="96"),
    "every prune through the multi-kernel path": dict(ALWAYS, BSLV_K2_LDS="64"),
}


class ride_hooks:
    """the engine's hooks of test_poly_modes_gpu plus the three variables of the switch (read by bslv_poly_create)"""

    def __init__(self, env, ride, g=None, t=None):
        self.h = hooks(env)
        self.mine = {"BSLV_R2_RIDE": "1" if ride else "0"}
        if g is not None:
            self.mine["BSLV_R2_RIDE_G"] = str(g)           # cap of the classifying workgroups
        if t is not None:
            self.mine["BSLV_R2_RIDE_T"] = str(t)           # threads of each that work (default 256)

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in RIDE_VARS}
        os.environ.update(self.mine)
        self.h.__enter__()

    def __exit__(self, *a):
        self.h.__exit__(*a)
        for k in RIDE_VARS:
            os.environ.pop(k, None)
        for k, v in self.old.items():
            if v is not None:
                os.environ[k] = v


def engine_run(q, D, k0, env, ride, g=None, t=None):
    with ride_hooks(env, ride, g, t):
        G = PolyEngine(q, 0, None)
        rcs = [G.add(D[i], 0) for i in range(k0)]
        assert G.init() == 0
        rcs += list(G.add_cuts(D[k0:], None))
        G.dual_adjacency()
        d = G.dump()
        st = G.rounds2_stats()
        health = G.rounds2_health()
        G.close()
    return [int(r) for r in rcs], d, st, health


def assert_bitwise(a, b, what):
    rca, da, sta, _ = a
    rcb, db, stb, _ = b
    assert rca == rcb, what
    for key in DUMP_KEYS:
        assert da[key].shape == db[key].shape and np.array_equal(da[key].view(np.uint8), db[key].view(np.uint8)), (what, key)
    assert sta == stb, (what, sta, stb)


@functools.lru_cache(maxsize=None)
def oracle_canonical(idx):
    name, q, D, k0 = CASES[idx]
    O = ph.FlatPoly("oracle", q, 0, None)
    ph.run_sequence(O, D, None, k0)
    O.dual_adjacency()
    exp = ph.canonical(O.dump())
    O.close()
    return exp


CASES = _r2_cases()
# chunks of 1024 cuts (nw = nwp = 32: 8 vertices per pass of a classifying workgroup, 32 with all 1024 threads at work) need more than a thousand cuts in one batch
CASES.append(("tangent q3, 1100 cuts", 3, np.vstack([ph.tangent_halfspaces(3, 6, 48), ph.tangent_halfspaces(3, 1100, 148)]), 6))
# dimension 11: the D = 0 instance of the kernel (dimensions 2..10 have instances of their own)
CASES.append(("truncated simplex q11",) + (11,) + truncated_simplex(11, 48, 5))
BY_NAME = {c[0]: i for i, c in enumerate(CASES)}


@pytest.mark.parametrize("idx", range(len(_r2_cases())), ids=lambda i: CASES[i][0])
def test_ride_along_builds_the_same_polyhedron_bit_for_bit(idx):
    """(a) every polyhedron of _r2_cases in five arms of the rounds: the dump and the return codes with the classification riding
    along equal those of the two launches bit for bit, and the polyhedron is the oracle's"""
    name, q, D, k0 = CASES[idx]
    exp = oracle_canonical(idx)
    for arm, env in ARMS.items():
        on = engine_run(q, D, k0, env, True)
        off = engine_run(q, D, k0, env, False)
        assert on[2]["cuts"] > 0 and on[2]["rounds"] > 0, (arm, on[2])
        assert on[3]["late_left"] == 0 and off[3]["late_left"] == 0, (arm, on[3], off[3])
        if "multi-kernel" in arm:
            assert on[2]["fallback_prunes"] > 0, (arm, on[2])
        assert_bitwise(on, off, arm)
        ph.assert_same(ph.canonical(on[1]), exp)
        ph.assert_same(ph.canonical(off[1]), exp)


# (b) shape edges of r2_classify3_body in the workgroups of the prunes' launch, with 256 (the default) and with all 1024 threads of
# a workgroup at work: nwp = nw rounded up to a power of two lanes per vertex
SHAPES = [
    ("tangent q4", "32"),                  # nw = 1, nwp = 1: 256 / 1024 vertices per workgroup
    ("tangent q4", "64"),                  # nw = 2, nwp = 2
    ("tangent q4", "96"),                  # nw = 3, nwp = 4: one idle lane in four
    ("crowded q5", "80"),                  # nw = 3 with a last word of 16 cuts
    ("tangent q3, 1100 cuts", "1024"),     # nw = nwp = 32
    ("truncated simplex q11", "1024"),     # the D = 0 instance (48 cuts: nw = nwp = 2)
]


@pytest.mark.parametrize("case,chunk", SHAPES, ids=lambda v: str(v))
def test_ride_along_at_the_shape_edges_of_the_classification(case, chunk):
    idx = BY_NAME[case]
    name, q, D, k0 = CASES[idx]
    env = dict(ALWAYS, BSLV_CHUNK_CUTS=chunk)
    on = engine_run(q, D, k0, env, True)
    off = engine_run(q, D, k0, env, False)
    assert on[2]["cuts"] > 0 and on[2]["rounds"] > 0, on[2]
    assert_bitwise(on, off, "switch")
    assert_bitwise(on, engine_run(q, D, k0, env, True, t=1024), "1024 threads")
    # one classifying workgroup strides over all new vertices of a round
    assert_bitwise(on, engine_run(q, D, k0, env, True, g=1), "G = 1")
    assert_bitwise(on, engine_run(q, D, k0, env, True, g=1, t=1024), "G = 1, 1024 threads")
    assert_bitwise(on, engine_run(q, D, k0, env, True, g=2, t=64), "G = 2, 64 threads")
    ph.assert_same(ph.canonical(on[1]), oracle_canonical(idx))


@pytest.mark.parametrize("idx", [BY_NAME["tangent q3"], BY_NAME["crowded q4"], BY_NAME["truncated cube q5"]], ids=lambda i: CASES[i][0])
def test_result_does_not_depend_on_the_number_of_classifying_workgroups(idx):
    """the classifying workgroups capped at 1 and at 3 (debug_set key 19 through its environment variable): the grid stride covers
    every new vertex, in both selection rules"""
    name, q, D, k0 = CASES[idx]
    for env in (dict(ALWAYS), dict(ALWAYS, BSLV_R2_MIS="0")):
        ref = engine_run(q, D, k0, env, True)
        for g in (1, 3):
            assert_bitwise(ref, engine_run(q, D, k0, env, True, g=g), (env, g))


def test_the_switch_through_debug_set():
    """debug_set keys 18 (the switch), 19 (cap of the classifying workgroups) and 20 (threads of each that work) do what the environment
    variables do"""
    name, q, D, k0 = CASES[BY_NAME["tangent q4"]]
    ref = engine_run(q, D, k0, ALWAYS, True)
    for key, value in ((18, 0), (19, 1), (20, 1024)):
        with ride_hooks(ALWAYS, True):
            G = PolyEngine(q, 0, None)
            G.debug_set(key, value)
            rcs = [G.add(D[i], 0) for i in range(k0)]
            assert G.init() == 0
            rcs += list(G.add_cuts(D[k0:], None))
            G.dual_adjacency()
            got = ([int(r) for r in rcs], G.dump(), G.rounds2_stats(), G.rounds2_health())
            G.close()
        assert_bitwise(ref, got, (key, value))


def _smid_steps(steps, ride):
    from bensolve_amd import synth
    from bensolve_amd.benson import BensonEngine
    with ride_hooks({}, ride):
        prob = synth.CONFIGS["S-mid"]()
        eng = BensonEngine(prob, eps=1e-7, pool_slots=2 * 1024 + 64)
        assert eng.start() == 0
        for _ in range(steps):
            nl, nt = eng.collect(1024, 0, 1)
            rec, piv, ls = eng.solve_local(nl)
            eng.apply(rec)
        d = eng.poly_dump()
        st = eng.poly_call("rounds2_stats")
        health = eng.poly_call("rounds2_health")
        eng.close()
    return d, st, health


def test_smid_benson_steps_identical_with_and_without_the_ride_along():
    """(c) three steps of the bench workload at batch 1024: the polyhedron, the counts of the rounds and their health"""
    on, off = _smid_steps(3, True), _smid_steps(3, False)
    assert on[1]["rounds"] > 0 and on[1]["cuts"] > 0, on[1]
    assert on[1] == off[1], (on[1], off[1])
    assert on[2]["late_left"] == 0 and off[2]["late_left"] == 0, (on[2], off[2])
    for key in DUMP_KEYS:
        assert on[0][key].shape == off[0][key].shape and np.array_equal(on[0][key].view(np.uint8), off[0][key].view(np.uint8)), key
