"""Two changes inside the launch of a round's prunes (k_r2_prune_classify), each behind a switch, neither of which may change a bit of
the polyhedron:

A. A large prune is worked in parts (BSLV_R2_SPLIT, _MIN, _PARTS, _H): helper workgroups of the same launch take a share of the rows
   of its pair phase and OR their words into the prune's bitmap in global memory.  The bitmap is a set and k_r2_k2emit emits from it
   in order, so the edge list must be the one of BSLV_R2_SPLIT=0 byte for byte -- with the split forced on every prune of two members
   or more, with 2, 3 and 4 parts, with a pool of 1, 3 and 32 helpers (too few for all prunes / enough), beside prunes that ask for
   their multi-kernel fallback, and in rounds that are declined or find the device halted.
B. The workgroups that classify a round's new vertices read the chunk's halfspaces from an image in their LDS (BSLV_R2_RIDE_LDS): same
   operands in the same order, so the class words -- and with them everything -- must equal BSLV_R2_RIDE_LDS=0 bit for bit."""
import os
import functools
import numpy as np
import pytest

import poly_harness as ph
from bensolve_amd.poly import PolyEngine
from test_poly_modes_gpu import hooks
from test_r2_ride_gpu import CASES, BY_NAME, ARMS, ALWAYS, DUMP_KEYS, SHAPES, oracle_canonical

pytestmark = pytest.mark.gpu

MY_VARS = ("BSLV_R2_SPLIT", "BSLV_R2_SPLIT_MIN", "BSLV_R2_SPLIT_PARTS", "BSLV_R2_SPLIT_H", "BSLV_R2_RIDE_LDS")
OFF = {"BSLV_R2_SPLIT": "0", "BSLV_R2_RIDE_LDS": "0"}                     # the launch as it was before either change
SPLIT_OFF = {"BSLV_R2_SPLIT": "0"}


def forced(parts, pool):
    """every prune of two members or more in `parts` parts, from a pool of `pool` helpers"""
    return {"BSLV_R2_SPLIT": "1", "BSLV_R2_SPLIT_MIN": "2", "BSLV_R2_SPLIT_PARTS": str(parts), "BSLV_R2_SPLIT_H": str(pool)}


class my_hooks:
    """the engine's hooks of test_poly_modes_gpu plus the variables of the two switches (read by bslv_poly_create)"""

    def __init__(self, env, mine):
        self.h, self.mine = hooks(env), mine

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in MY_VARS}
        os.environ.update(self.mine)
        self.h.__enter__()

    def __exit__(self, *a):
        self.h.__exit__(*a)
        for k in MY_VARS:
            os.environ.pop(k, None)
        for k, v in self.old.items():
            if v is not None:
                os.environ[k] = v


def finish(G, rcs):
    G.dual_adjacency()
    out = ([int(r) for r in rcs], G.dump(), G.rounds2_stats(), G.rounds2_health(), G.split_stats())
    G.close()
    return out


def engine_run(q, D, k0, env, mine):
    with my_hooks(env, mine):
        G = PolyEngine(q, 0, None)
        rcs = [G.add(D[i], 0) for i in range(k0)]
        assert G.init() == 0
        rcs += list(G.add_cuts(D[k0:], None))
        return finish(G, rcs)


def assert_bitwise(a, b, what):
    assert a[0] == b[0], what
    for key in DUMP_KEYS:
        assert a[1][key].shape == b[1][key].shape and np.array_equal(a[1][key].view(np.uint8), b[1][key].view(np.uint8)), (what, key)
    assert a[2] == b[2], (what, a[2], b[2])
    assert a[3]["late_left"] == 0 and b[3]["late_left"] == 0, (what, a[3], b[3])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=lambda i: CASES[i][0])
def test_rounds_bit_identical_with_the_split_forced(idx):
    """the ten polyhedra of the mode tests with every prune of two members or more split (one pair; more parts than rows; member counts
    that are no multiple of 16 T; a pool of 1 or 3 helpers, too small for the prunes of a round): dumps, return codes and the counts of
    the rounds equal those without the split byte for byte"""
    name, q, D, k0 = CASES[idx]
    off = engine_run(q, D, k0, ALWAYS, SPLIT_OFF)
    assert off[2]["cuts"] > 0 and off[2]["rounds"] > 0 and off[4]["split_prunes"] == 0, (off[2], off[4])
    for parts in (2, 3, 4):
        for pool in (1, 3, 32):
            on = engine_run(q, D, k0, ALWAYS, forced(parts, pool))
            assert on[4]["split_prunes"] > 0 and on[4]["helper_parts"] >= on[4]["split_prunes"], (parts, pool, on[4])
            assert on[4]["helper_parts"] <= (parts - 1) * on[4]["split_prunes"], (parts, pool, on[4])
            assert_bitwise(on, off, (parts, pool))
    if idx < 8:                        # (the two large ones are held against the oracle in test_r2_ride_gpu)
        ph.assert_same(ph.canonical(off[1]), oracle_canonical(idx))


# one deep cut through the middle of a random polytope, as in test_poly_window_gpu: (q, N, seed) of tangent_halfspaces and the
# members of the new facet on oracle/poly_dd.c; 561 members are more than one workgroup takes (fallback -1)
DEEP = {"q4, 234 members": (4, 300, 1, 234), "q5, 423 members": (5, 120, 1, 423), "q5, 561 members": (5, 160, 1, 561)}


def _deep_input(name):
    q, N, seed = DEEP[name][:3]
    extra = np.zeros(q)
    extra[0] = 1e6                       # the halfspace y_0 >= -1e-6
    return q, ph.tangent_halfspaces(q, N, seed), extra, ph.tangent_halfspaces(q, 40, seed + 50)


def _last_facet_members(d, slot):
    live = d["pu"].astype(bool)
    I = d["I"]
    return int((live[I[:, 0]] & (I[:, 1] == slot)).sum())


@functools.lru_cache(maxsize=None)
def _deep_oracle(name, beside):
    q, D, extra, more = _deep_input(name)
    O = ph.FlatPoly("oracle", q, 0, None)
    ph.run_sequence(O, D)
    assert O.add(extra, 0) == 0
    if beside:
        for y in more:
            O.add(y, 0)
        O.dual_adjacency()
    d = O.dump()
    O.close()
    return d


def _deep_engine(name, beside, mine):
    q, D, extra, more = _deep_input(name)
    with my_hooks(ALWAYS, mine):
        G = PolyEngine(q, 0, None)
        rcs = ph.run_sequence(G, D)
        rcs += list(G.add_cuts(np.vstack([extra[None, :], more]) if beside else extra[None, :], None))
        return finish(G, rcs)


@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_cut_split_beside_unsplit_prunes(name):
    """a facet of several hundred members at the default threshold (from 64 members on, 1 + members / 64 parts, at most 4) in one chunk
    with 40 shallow cuts, whose prunes are not split: the run equals the one without the split byte for byte, and the polyhedron is
    that of oracle/poly_dd.c.  The oracle is compared as sets of slots, not slot for slot: rounds need a chunk of several cuts (a
    lone cut goes through the single-cut pipeline and never reaches the rounds' prunes), and a round of several cuts numbers its new
    vertices in the order of the edges they lie on, not cut by cut -- with or without the split."""
    nm = DEEP[name][3]
    do = _deep_oracle(name, False)
    assert _last_facet_members(do, len(do["du"]) - 1) == nm
    on, off = _deep_engine(name, True, {}), _deep_engine(name, True, SPLIT_OFF)
    assert on[2]["cuts"] > 1, on[2]
    if nm <= 512:
        assert on[4]["split_prunes"] >= 1 and on[4]["helper_parts"] >= 3 and on[2]["cuts"] > on[4]["split_prunes"], (on[4], on[2])
    else:
        assert on[2]["fallback_prunes"] >= 1, on[2]
    assert_bitwise(on, off, "beside 40 shallow cuts")
    ph.assert_same(ph.canonical(on[1]), ph.canonical(_deep_oracle(name, True)))


@pytest.mark.parametrize("lds", ["64", "66000", "70000"])
@pytest.mark.parametrize("case", ["tangent q4", "crowded q5", "truncated cube q5"])
def test_split_prunes_that_ask_for_the_multi_kernel_fallback(case, lds):
    """a small k2_lds while every prune is split: with 64 bytes not even the pair bitmap fits (-2, every prune falls back); with 66000
    the hash table of a prune of up to ~85 members fits and its bit matrix never does (-4 in every part), larger ones count in global
    memory and are not split; with 70000 the bit matrix of the larger prunes does not fit, beside prunes that are worked in parts.
    All parts return, the prune's own workgroup reports, the multi-kernel path builds the same edges"""
    name, q, D, k0 = CASES[BY_NAME[case]]
    env = dict(ALWAYS, BSLV_K2_LDS=lds)
    off = engine_run(q, D, k0, env, SPLIT_OFF)
    on = engine_run(q, D, k0, env, forced(3, 32))
    if lds == "70000":
        assert on[4]["split_prunes"] > 0, on[4]
    else:
        assert on[2]["fallback_prunes"] > 0, on[2]
    assert_bitwise(on, off, lds)
    ph.assert_same(ph.canonical(on[1]), oracle_canonical(BY_NAME[case]))


@pytest.mark.parametrize("case", ["tangent q3", "crowded q4", "truncated cube q4"])
def test_split_in_every_arm_of_the_rounds(case):
    """the arms of test_r2_ride_gpu with every prune split: the local-minima rule, nothing queued ahead, chunks of 96 (rounds that are
    declined, and rounds queued ahead that find the device halted: every role of the launch returns at once), every prune through
    the multi-kernel path"""
    name, q, D, k0 = CASES[BY_NAME[case]]
    for arm, env in ARMS.items():
        off = engine_run(q, D, k0, env, OFF)
        on = engine_run(q, D, k0, env, forced(3, 3))
        assert_bitwise(on, off, arm)
        if "multi-kernel" not in arm:
            assert on[4]["split_prunes"] > 0, (arm, on[4])


# B: the shape edges of the classification (nw = 1, 2, 3, 3 with a short last word, 32, the D = 0 instance), a chunk of 1024 cuts
# in dimension 5 (the image takes 66 KB: fits), and an LDS too small for any image (the path through global memory; the prunes fall back)
LDS_SHAPES = [(c, k, {}) for c, k in SHAPES] + [("tangent q5, 1100 cuts", "1024", {}), ("tangent q5, 1100 cuts", "1024", {"BSLV_K2_LDS": "64"})]
Q5_BIG = ("tangent q5, 1100 cuts", 5, np.vstack([ph.tangent_halfspaces(5, 8, 3), ph.tangent_halfspaces(5, 1100, 103)]), 8)


@pytest.mark.parametrize("case,chunk,extra", LDS_SHAPES, ids=lambda v: str(v))
def test_classification_from_the_lds_image_is_bit_identical(case, chunk, extra):
    name, q, D, k0 = Q5_BIG if case == Q5_BIG[0] else CASES[BY_NAME[case]]
    env = dict(ALWAYS, BSLV_CHUNK_CUTS=chunk, **extra)
    on = engine_run(q, D, k0, env, {"BSLV_R2_RIDE_LDS": "1", "BSLV_R2_SPLIT": "0"})
    off = engine_run(q, D, k0, env, OFF)
    assert on[2]["cuts"] > 0 and on[2]["rounds"] > 0, on[2]
    assert_bitwise(on, off, "BSLV_R2_RIDE_LDS")
    # ... and with everything on, at the defaults
    assert_bitwise(engine_run(q, D, k0, env, {}), off, "both, defaults")


def test_the_switches_through_debug_set():
    """debug_set keys 22 (LDS image), 23 (split), 24 (threshold), 25 (parts) and 26 (helpers) do what the environment variables do"""
    name, q, D, k0 = CASES[BY_NAME["tangent q4"]]
    ref = engine_run(q, D, k0, ALWAYS, OFF)
    for keys, split in ((((22, 0), (23, 0)), False), (((24, 2), (25, 4), (26, 5)), True)):
        with my_hooks(ALWAYS, {}):
            G = PolyEngine(q, 0, None)
            for key, value in keys:
                G.debug_set(key, value)
            rcs = [G.add(D[i], 0) for i in range(k0)]
            assert G.init() == 0
            rcs += list(G.add_cuts(D[k0:], None))
            got = finish(G, rcs)
        assert (got[4]["split_prunes"] > 0) == split, (keys, got[4])
        assert_bitwise(ref, got, keys)


def _smid_steps(steps, mine):
    from bensolve_amd import synth
    from bensolve_amd.benson import BensonEngine
    with my_hooks({}, mine):
        prob = synth.CONFIGS["S-mid"]()
        eng = BensonEngine(prob, eps=1e-7, pool_slots=2 * 1024 + 64)
        assert eng.start() == 0
        recs = []
        for _ in range(steps):
            nl, nt = eng.collect(1024, 0, 1)
            rec, piv, ls = eng.solve_local(nl)
            eng.apply(rec)
            recs.append(np.array(rec, copy=True))
        d = eng.poly_dump()
        st = eng.poly_call("rounds2_stats")
        health = eng.poly_call("rounds2_health")
        sp = eng.poly_call("split_stats")
        eng.close()
    return d, st, health, sp, recs


def test_smid_benson_steps_identical_with_everything_on_and_off():
    """three steps of the bench workload at batch 1024, both changes at their defaults against both off: the LP records of every step,
    the polyhedron, the counts of the rounds and their health; the workload has prunes above the threshold"""
    on, off = _smid_steps(3, {}), _smid_steps(3, OFF)
    assert on[1]["rounds"] > 0 and on[1]["cuts"] > 0, on[1]
    assert on[1] == off[1], (on[1], off[1])
    assert on[2]["late_left"] == 0 and off[2]["late_left"] == 0, (on[2], off[2])
    assert on[3]["split_prunes"] > 0 and off[3]["split_prunes"] == 0, (on[3], off[3])
    for a, b in zip(on[4], off[4]):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for key in DUMP_KEYS:
        assert on[0][key].shape == off[0][key].shape and np.array_equal(on[0][key].view(np.uint8), off[0][key].view(np.uint8)), key
