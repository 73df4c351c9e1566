"""GPU: bslv_poly_compact -- the live elements renumbered 0 .. live-1 in slot order, their incidence lists packed (include/bslv_hip.h).

Cases (generators of poly_harness.py, the instances and k0 of test_poly_dims_gpu.py): truncated simplex q = 3, 5, 11, the shuffled
cross-polytope q = 8 (lists longer than LONGN = 64: the wave path of the list copy, slack that is reset), tangent halfspaces q = 7,
the ideal cone q = 11 (ideal elements, the apex) and the degenerate simplex q = 11.  The compaction point lies after
(len + k0) // 2 dual points; the cuts behind k0 go through bslv_poly_add_cuts in two calls, in both batch modes.  The CPU oracle has
at that point 19 / 41 / 155 / 5 032 / 2 702 / 47 / 401 slots with a dead share of 0.37 / 0.27 / 0.15 / 0.96 / 0.55 / 0.11 / 0.16, so
every case must remove something and find at least a tenth of its slots dead.

Compared with rtol = atol = 0: the canonical dump before and after the call, and the finished polyhedron of a run with the call in
the middle against the same run without it.  Against the oracle: poly_harness.assert_same at its defaults, as test_poly_dims_gpu.py
compares (it documents no allowance for these cases, so there is none here)."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import poly_harness as ph
from bensolve_amd._lib import load_library
from bensolve_amd.poly import PolyEngine, _bind

pytestmark = pytest.mark.gpu

NAMES = ["truncated simplex q3", "truncated simplex q5", "truncated simplex q11", "cross-polytope q8, shuffled", "tangent q7",
         "ideal cone q11", "degenerate simplex q11"]


def case(name):
    """(q, vals, ideals, apex, k0) -- test_poly_dims_gpu.CASES, which builds them as the table in the issue does"""
    from test_poly_dims_gpu import CASES
    q, vals, ideals, apex, _, k0 = CASES[name]
    vals = np.asarray(vals, float)
    idl = np.zeros(len(vals), np.int32) if ideals is None else np.asarray(ideals, np.int32)
    return q, vals, idl, apex, k0


def start(name, mode):
    """the engine of a case at its compaction point"""
    q, vals, idl, apex, k0 = case(name)
    mid = (len(vals) + k0) // 2
    G = PolyEngine(q, 0, None)
    if apex:
        G.dual0_apex()
    G.set_batch_mode(mode)
    for i in range(k0):
        G.add(vals[i], int(idl[i]))
    assert G.init() == 0
    G.add_cuts(vals[k0:mid], idl[k0:mid])
    return G, vals[mid:], idl[mid:]


def finish(G, vals, idl):
    G.add_cuts(vals, idl)
    G.dual_adjacency()
    d, ck = G.dump(), G.check()
    G.close()
    assert ck["clean"], ck
    return d


@functools.lru_cache(maxsize=None)
def plain_run(name, mode):
    """canonical result of the run WITHOUT a compaction; read-only for its users"""
    G, vals, idl = start(name, mode)
    return ph.canonical(finish(G, vals, idl))


def sha(can, decimals=7):
    h = hashlib.sha256()
    for k in sorted(can):
        v = can[k]
        if isinstance(v, np.ndarray):
            h.update(k.encode()); h.update(np.ascontiguousarray(np.round(v, decimals) + 0.0 if v.dtype.kind == "f" else v).tobytes())
        else:
            h.update(k.encode()); h.update(np.array(sorted(v), np.int64).tobytes())
    return h.hexdigest()


def figures_of(d):
    """[0] [1] [3] [4] of bslv_poly_garbage from a dump alone"""
    return len(d["pu"]), int(d["pu"].sum()), len(d["I"]), len(d["E"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_compaction_keeps_the_state_and_the_run_that_follows(name, mode):
    G, vals, idl = start(name, mode)
    before, ck0, g0 = G.dump(), G.check(), G.garbage()
    n2o, fig = G.compact()
    after, ck1, g1, st = G.dump(), G.check(), G.garbage(), G.last_compact_stats()
    nv0, live = len(before["pu"]), int(before["pu"].sum())
    print("%s, mode %d: %d slots, %d live (dead %.2f); pool %d -> %d words; bytes %d -> %d; %d us" % (
        name, mode, nv0, live, 1 - live / nv0, g0["pool_used"], g1["pool_used"], g0["bytes"], g1["bytes"], st["us"]))
    assert ck0["clean"], ck0
    assert ck1["clean"], ck1
    # not vacuous
    assert st["slots_removed"] == nv0 - live > 0 and (nv0 - live) / nv0 >= 0.10
    # the figures, against the dumps
    for g, d in ((g0, before), (g1, after)):
        assert (g["slots"], g["live"], g["pool_live"], g["edges"]) == figures_of(d)
    assert g0["pool_used"] >= g0["pool_live"] and g1["pool_used"] == g1["pool_live"] == g0["pool_live"]
    assert fig["out"] == g1["out"]
    assert st["pool_removed"] == g0["pool_used"] - g1["pool_used"] and st["bytes_returned"] == g0["bytes"] - g1["bytes"] >= 0
    # the map: -1 exactly on the dead slots, strictly increasing on the live ones, onto 0 .. live-1
    pu = before["pu"].astype(bool)
    assert len(n2o) == nv0 and np.all(n2o[~pu] == -1)
    assert np.array_equal(n2o[pu], np.arange(live))
    assert G.lib.bslv_poly_nprimal(G.h) == live == len(after["pu"]) and np.all(after["pu"] == 1)
    # coordinates and marks bit for bit, the edges row by row in their order, every list in its order
    assert np.array_equal(after["X"].view(np.uint64), before["X"][pu].view(np.uint64))
    assert np.array_equal(after["pi"], before["pi"][pu]) and np.array_equal(after["ps"], before["ps"][pu])
    assert np.array_equal(after["E"], n2o[before["E"]])
    Ib = before["I"].copy()
    Ib[:, 0] = n2o[Ib[:, 0]]
    assert np.array_equal(after["I"], Ib)
    for k in ("du", "di", "Y"):
        assert np.array_equal(after[k], before[k])
    ph.assert_same(ph.canonical(after), ph.canonical(before), rtol=0, atol=0)
    # a second call straight after: the identity, nothing removed, capacities unchanged
    n2o2, fig2 = G.compact()
    st2 = G.last_compact_stats()
    assert np.array_equal(n2o2, np.arange(live)) and fig2["out"] == g1["out"]
    assert st2["calls"] == 2 and st2["slots_removed"] == st2["pool_removed"] == st2["bytes_returned"] == 0
    assert st2["slots_removed_total"] == st["slots_removed"] and G.garbage()["out"] == g1["out"]
    # the run goes on as if nothing had happened
    got = ph.canonical(finish(G, vals, idl))
    ph.assert_same(got, plain_run(name, mode), rtol=0, atol=0)
    from test_poly_dims_gpu import oracle_canonical
    ph.assert_same(got, oracle_canonical(name))


def test_marks_survive():
    G, _, _ = start("tangent q7", 1)
    idx, val, ideal, cnt = G.unprocessed()
    assert cnt == len(idx) > 30
    G.mark(idx[::3])
    keep = np.ones(len(idx), bool)
    keep[::3] = False
    n2o, _ = G.compact()
    idx2, val2, ideal2, cnt2 = G.unprocessed()
    G.close()
    assert cnt2 == keep.sum()
    assert np.array_equal(idx2, n2o[idx[keep]])
    assert np.array_equal(val2.view(np.uint64), val[keep].view(np.uint64)) and np.array_equal(ideal2, ideal[keep])


def test_memory_is_handed_back():
    G, _, _ = start("cross-polytope q8, shuffled", 1)
    b0 = G.garbage()["out"][5]
    G.compact()
    b1, st = G.garbage()["out"][5], G.last_compact_stats()["out"]
    G.close()
    print("cross-polytope q8: %d -> %d bytes" % (b0, b1))
    assert b1 < b0 and st[3] == b0 - b1


def _with_compaction(name, mode):
    G, vals, idl = start(name, mode)
    G.compact()
    return ph.canonical(finish(G, vals, idl))


def test_poisoned_allocations():
    """tangent q = 7 with the compaction in the middle, in a process whose fresh device memory is 0x7F bytes (tests/test_fill_gpu.py):
    the same sets, by SHA-256 over the canonical dump, as on the memory every other test sees"""
    env = dict(os.environ, BSLV_FILL="0x7F")
    env.pop("BSLV_ALLOC_LOG", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
    assert "Memory access fault" not in p.stderr, p.stderr[-800:]
    assert p.returncode == 0, "rc %d\n%s" % (p.returncode, p.stderr[-1500:])
    row = json.loads(p.stdout.strip().splitlines()[-1])
    assert row["fill"] == "0x7F" and row["removed"] > 0
    assert row["sha256"] == sha(_with_compaction("tangent q7", 1)) == sha(plain_run("tangent q7", 1))


def test_arguments():
    lib = load_library()
    _bind(lib)
    lib.bslv_poly_compact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.bslv_poly_compact(None, None, None) == 2           # BSLV_E_ARG
    G = PolyEngine(3)
    n2o, fig = G.compact()                                        # before init(): nothing to do
    assert len(n2o) == 0 and fig["out"] == [0] * 6 and G.garbage()["out"] == [0] * 6
    G.add(np.array([1.0, 0.0, 0.0]))                              # (queued: still not initialised)
    n2o, fig = G.compact()
    assert len(n2o) == 0 and fig["out"] == [0] * 6 and G.last_compact_stats()["calls"] == 0
    G.close()


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    G, vals, idl = start("tangent q7", 1)
    G.compact()
    removed = G.last_compact_stats()["slots_removed"]
    print(json.dumps(dict(fill=os.environ.get("BSLV_FILL", "0"), removed=removed, sha256=sha(ph.canonical(finish(G, vals, idl))))), flush=True)
