"""The multi-kernel adjacency prune of a large new facet (k2_multi, row-tiled pair kernel) walks the pair space in windows: ranges
of row groups that are tested, scanned and emitted one after the other, with 64-bit virtual block ids on the host and ids relative
to the window on the device.  Whatever the window, the polyhedron must be the one a single pass builds, bit for bit -- and the one
oracle/poly_dd.c builds.  The index arithmetic beyond 2^32 blocks is run on its own (bslv_selftest_pair_blocks)."""
import functools
import hashlib
import os
import numpy as np
import pytest

import poly_harness as ph
from bensolve_amd._lib import BslvError
from bensolve_amd.poly import PolyEngine

pytestmark = pytest.mark.gpu

PB, PTI = 256, 8
DEFAULT_WINDOW = 0x7FFFFFF0


def pair_G(K):
    """pair blocks (one row, 256 columns) of rows with 1 .. K columns: sum of ceil(k / 256)"""
    f = K // PB
    return PB * f * (f + 1) // 2 + (K - PB * f) * (f + 1)


def pair_S(nm, i):
    """pair blocks in front of row i of a facet of nm members"""
    L = nm - 1
    return pair_G(L) - pair_G(L - min(i, L))


def greedy_windows(nm, window):
    """number of windows of the greedy rule: consecutive row groups while at most `window` blocks, at least one group"""
    ngroups = (nm - 1 + PTI - 1) // PTI
    n, ga = 0, 0
    while ga < ngroups:
        s0, g = pair_S(nm, ga * PTI), ga + 1
        while g < ngroups and pair_S(nm, (g + 1) * PTI) - s0 <= window:
            g += 1
        n, ga = n + 1, g
    return n


# one deep cut through the middle of a random polytope: (q, N, seed) of tangent_halfspaces, then members of the new facet,
# live vertices and edges afterwards on oracle/poly_dd.c
DEEP = {"q5": (5, 300, 1, 984, 4730, 11825), "q6": (6, 140, 2, 2272, 7649, 22947)}


def _deep_points(name):
    q, N, seed = DEEP[name][:3]
    extra = np.zeros(q)
    extra[0] = 1e6                       # the halfspace y_0 >= -1e-6
    return q, ph.tangent_halfspaces(q, N, seed), extra


def _last_facet_members(d):
    live = d["pu"].astype(bool)
    I = d["I"]
    return int((live[I[:, 0]] & (I[:, 1] == len(d["du"]) - 1)).sum())


@functools.lru_cache(maxsize=None)
def _deep_oracle(name):
    q, D, extra = _deep_points(name)
    O = ph.FlatPoly("oracle", q, 0, None)
    ph.run_sequence(O, D)
    assert O.add(extra, 0) == 0
    d = O.dump()
    O.close()
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _deep_engine(name, window, noflags, lists, fm_min=2):
    q, D, extra = _deep_points(name)
    G = PolyEngine(q, 0, None)
    G.set_batch_mode(0)
    G.debug_set(0, 64)                   # every prune through the multi-kernel path
    G.debug_set(4, fm_min)               # 2: every facet takes the tiled path
    G.debug_set(16, noflags)
    G.debug_set(5, lists)
    G.set_prune_window(window)
    ph.run_sequence(G, D)
    assert G.add(extra, 0) == 0
    d = G.dump()
    paths, st = G.path_stats(), G.prune_window_stats()
    G.close()
    return d, paths, st


_first_arm = {}                          # input -> the dump of the first arm that ran: every arm equals it, so all equal each other


def _assert_deep_dump(name, d, arm):
    nm, nlive, nedges = DEEP[name][3:]
    do = _deep_oracle(name)
    assert _last_facet_members(do) == nm and _last_facet_members(d) == nm, (arm, _last_facet_members(d))
    assert int(d["pu"].sum()) == nlive and len(d["E"]) == nedges, (arm, int(d["pu"].sum()), len(d["E"]))
    for key in ("pu", "pi", "du", "di", "E", "I"):
        assert np.array_equal(do[key], d[key]), (arm, key)
    live = do["pu"].astype(bool)
    np.testing.assert_allclose(do["X"][live], d["X"][live], rtol=1e-12, atol=1e-12)
    ref = _first_arm.setdefault(name, d)
    for key in ("pu", "pi", "ps", "X", "du", "di", "Y", "E", "I", "DE"):
        assert np.array_equal(ref[key], d[key]), (arm, key)


@pytest.mark.parametrize("lists", [1, 0], ids=["member_lists", "full_scan"])
@pytest.mark.parametrize("noflags", [0, 1], ids=["flags", "noflags"])
@pytest.mark.parametrize("name", sorted(DEEP))
def test_deep_cut_is_the_oracles_in_every_window(name, noflags, lists):
    """a facet of 984 (2396 pair blocks, 123 row groups) / 2272 members (11 223 blocks, 284 row groups) pruned in one window, in
    windows of one row group, of 100 and of 1000 blocks: slots, edges and incidence lists of oracle/poly_dd.c bit for bit,
    coordinates at 1e-12, and every arm equal to every other bit for bit"""
    nm = DEEP[name][3]
    blocks, first_group = pair_G(nm - 1), pair_S(nm, PTI)
    assert (nm, blocks, first_group) in ((984, 2396, 32), (2272, 11223, 72))
    for window in (0, 1, 100, 1000, 10 ** 9):
        arm = (name, window, noflags, lists)
        d, paths, st = _deep_engine(name, window, noflags, lists)
        _assert_deep_dump(name, d, arm)
        assert paths["prune_fallbacks"] > 0, (arm, paths)
        assert (paths["member_list_prunes"] > 0) == bool(lists), (arm, paths)
        if window in (1, 100, 1000):
            widest = max(window, first_group)
            assert st[0] >= 1 and st[1] >= -(-blocks // widest), (arm, st)
            assert st[1] >= greedy_windows(nm, window), (arm, st)
            assert 0 < st[2] <= widest, (arm, st)
        else:
            assert st[0] == 0 and st[1] == 0 and st[2] == blocks, (arm, st)


def test_untiled_path_ignores_the_window():
    """no facet is 'large' (debug key 4): the one-dimensional pair launch numbers the blocks of the whole facet, window or not"""
    d, paths, st = _deep_engine("q5", 1, 0, 1, fm_min=1 << 30)
    _assert_deep_dump("q5", d, "untiled")
    assert paths["prune_fallbacks"] > 0 and paths["member_list_prunes"] == 0, paths
    assert st == [0, 0, 0], st


def test_real_degenerate_cuts_in_windows_of_one_row_group():
    """~2000 cuts of the bench workload S-mid (extreme directions with long incidence lists, degenerate points), replayed one at a
    time with every prune on the tiled multi-kernel path: windows of one row group give the dump of one window bit for bit"""
    from test_poly_modes_gpu import _smid_cut_sequence
    q, c, Y, _ = _smid_cut_sequence(6)
    out = {}
    for window in (0, 1):
        G = PolyEngine(q, 1, c)
        G.set_batch_mode(0)
        G.debug_set(0, 64)
        G.debug_set(4, 2)
        G.set_prune_window(window)
        for k in range(1, q + 1):
            G.add(Y[k], 0)
        assert G.init() == 0
        rest = Y[q + 1:]
        for b0 in range(0, len(rest), 256):
            G.add_cuts(rest[b0:b0 + 256], None)
        out[window] = (G.dump(), G.path_stats(), G.prune_window_stats())
        G.close()
        assert len(rest) > 1500 and out[window][1]["member_list_prunes"] > 1500, out[window][1:]
    for key in ("pu", "pi", "ps", "X", "du", "di", "Y", "E", "I", "DE"):
        assert np.array_equal(out[0][0][key], out[1][0][key]), key
    assert out[0][2][0] == 0, out[0][2]
    assert out[1][2][0] > 1000 and out[1][2][1] > 2 * out[1][2][0], out[1][2]


def test_window_from_the_environment_through_the_driver():
    """BSLV_K2_WINDOW reaches the polyhedron engine that bslv_benson_create makes; six steps of S-small with every prune on the
    tiled multi-kernel path give the same polyhedron with windows of one row group"""
    from bensolve_amd import synth
    from bensolve_amd.benson import BensonEngine
    from test_poly_modes_gpu import hooks
    prob = synth.CONFIGS["S-small"]()

    def run(env):
        assert "BSLV_K2_WINDOW" not in os.environ
        try:
            with hooks(env):
                eng = BensonEngine(prob, eps=1e-7, pool_slots=4 * 256 + 64)
        finally:
            os.environ.pop("BSLV_K2_WINDOW", None)
        eng.poly_call("debug_set", 4, 2)
        assert eng.start() == 0
        eng.run(256, max_steps=6)
        d = eng.poly_dump()
        res = (eng.poly_call("get_prune_window"), eng.poly_call("prune_window_stats"), eng.poly_call("path_stats"), eng.poly_call("rounds2_stats"))
        eng.close()
        h = hashlib.sha256()
        for key in ("pu", "pi", "ps", "X", "du", "di", "Y", "E", "I"):
            h.update(np.ascontiguousarray(d[key]).tobytes())
        return (h.hexdigest(), int(d["pu"].sum()), len(d["E"])), res

    one, r1 = run({"BSLV_K2_LDS": "64"})
    win, rw = run({"BSLV_K2_WINDOW": "1", "BSLV_K2_LDS": "64"})
    assert one == win and one[1] > 100, (one, win)
    assert r1[0] == DEFAULT_WINDOW and rw[0] == 1
    assert r1[2]["prune_fallbacks"] + r1[3]["fallback_prunes"] > 0, r1
    # (the facets of these six steps fit one row group: what is checked here is the way of the switch)
    assert r1[1][0] == 0 and r1[1][2] > 0 and rw[1][2] == r1[1][2], (r1, rw)


@pytest.mark.parametrize("nm,least", [(1663073, 3), (3000000, 9)])
def test_index_arithmetic_beyond_32_bits(nm, least):
    """facets whose pair space holds more than 2^32 blocks (the first is the facet that stopped S-degenerate at q = 10): 200 000
    hashed pairs go to (window, relative id) and back without a mismatch, the relative ids fit 31 bits"""
    out = PolyEngine.selftest_pair_blocks(nm, 0, 200000)
    total = pair_G(nm - 1)
    assert total > 2 ** 32 and out[1] == total, (out, total)
    assert out[2] == 0, out
    assert out[0] == greedy_windows(nm, DEFAULT_WINDOW) and out[0] >= least and out[0] >= -(-total // DEFAULT_WINDOW), out
    assert 0 <= out[3] < 2 ** 31 and out[3] < DEFAULT_WINDOW, out


def test_index_arithmetic_small_facets():
    out = PolyEngine.selftest_pair_blocks(984, 100, 50000)
    assert out == [greedy_windows(984, 100), 2396, 0, out[3]] and out[0] >= 24 and out[3] < 100, out
    assert PolyEngine.selftest_pair_blocks(2, 0, 1) == [1, 1, 0, 0]
    assert PolyEngine.selftest_pair_blocks(984, 1, 50000)[:3] == [123, 2396, 0]          # one row group per window
    for bad in ((1, 0, 10), (984, -1, 10), (984, 0, 0)):
        with pytest.raises(BslvError, match="error 2"):
            PolyEngine.selftest_pair_blocks(*bad)


def test_window_arguments():
    G = PolyEngine(3, 0, None)
    assert G.get_prune_window() == DEFAULT_WINDOW
    G.set_prune_window(100)
    assert G.get_prune_window() == 100
    with pytest.raises(BslvError, match="error 2"):
        G.set_prune_window(-1)
    assert G.get_prune_window() == 100
    G.set_prune_window(0)
    assert G.get_prune_window() == DEFAULT_WINDOW
    assert G.prune_window_stats() == [0, 0, 0]
    G.close()
