"""The batched classification runs over a device-side list of the LIVE element slots; dead slots must still read as untouched.

Through both test entry points (bslv_poly_classify_batch, bslv_poly_classify_batch_touch), on a q = 3 polyhedron whose slot
array is mostly dead: for live slots the class words, touch counts, first touched halfspace and the any-MINUS verdicts equal a
NumPy recomputation with the kernel's thresholds (alpha +- POLY_EPS, 0 +- POLY_EPS for ideal elements); for dead slots every
class word is zero, tc == 0 and t1 == -1.  No live element lies within 1e-6 of a threshold (asserted), so nothing hinges on
FMA rounding.

The polyhedron: 4 halfspaces, the initial approximation, then 60 more -- seeded random unit normals tilted towards +z, so that
the polyhedron keeps a recession cone (live ideal directions), the last 24 of them 1.6 times as deep, so that they cut away
nearly everything the first 36 built (long runs of dead slots).  Seed 1 was chosen with oracle/poly_dd.c on the CPU: 342 slots,
54 live (7 of them ideal), two aligned runs of 64 dead slots, four mixed ones; the tests assert what they need of that from
bslv_poly_get_primal's flags."""
import numpy as np
import pytest

import poly_harness as ph
from bensolve_amd.poly import PolyEngine

pytestmark = pytest.mark.gpu

Q = 3
POLY_EPS = 1e-9
SEED, N_INIT, N_FIRST, N_DEEP, N_MORE = 1, 4, 36, 24, 12


def cut_points(seed=SEED):
    """dual vertices d (halfspace d.y >= -1 through cone_polar): the 4 + 60 that build the polyhedron, then 12 deeper ones"""
    rng = np.random.default_rng(seed)
    D = rng.normal(size=(N_INIT + N_FIRST + N_DEEP + N_MORE, Q))
    D[:, 2] = np.abs(D[:, 2]) + 0.6
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    D[N_INIT + N_FIRST:N_INIT + N_FIRST + N_DEEP] *= 1.6
    D[N_INIT + N_FIRST + N_DEEP:] *= 2.2
    return D[:N_INIT + N_FIRST + N_DEEP], D[N_INIT + N_FIRST + N_DEEP:]


def build(P):
    D, more = cut_points()
    ph.run_sequence(P, D, init_after=N_INIT)
    return more


def primal(P):
    d = P.dump()
    return d["X"], d["pu"].astype(bool), d["pi"].astype(bool)


def halfspaces(X, used, ideal, B, first=None, seed=7):
    """B halfspaces (normal, alpha) that split the live elements, each 1e-3 off a live vertex and with no live element within
    2e-6 of its plane (candidates that have one are drawn again); `first` (if given) go in front as they are"""
    rng = np.random.default_rng(seed)
    verts = np.nonzero(used & ~ideal)[0]
    H = [] if first is None else [np.asarray(h, float) for h in first]
    while len(H) < B:
        n = rng.normal(size=Q)
        h = np.append(n, n @ X[verts[rng.integers(len(verts))]] - 1e-3)
        s = X[used] @ n - np.where(ideal[used], 0.0, h[Q])
        if np.abs(s).min() > 2e-6:
            H.append(h)
    return np.array(H[:B])


def expected(X, used, ideal, H):
    """(words, tc, t1, anyminus) as the kernel defines them; also asserts that no live element is within 1e-6 of a threshold"""
    B, nv = len(H), len(X)
    s = np.zeros((B, nv))
    for k in range(Q):
        s = s + H[:, k:k + 1] * X[None, :, k]
    a = np.where(ideal[None, :], 0.0, H[:, Q:Q + 1])
    gap = np.minimum(np.abs(s - (a + POLY_EPS)), np.abs(s - (a - POLY_EPS)))
    assert gap[:, used].min() > 1e-6, "a live element lies within 1e-6 of a threshold: choose other halfspaces"
    cls = np.where(s > a + POLY_EPS, 3, np.where(s > a - POLY_EPS, 2, 1))
    cls = np.where(used[None, :], cls, 0)
    words = np.zeros(((B + 31) // 32, nv), np.uint64)
    for b in range(B):
        words[b // 32] |= cls[b].astype(np.uint64) << np.uint64(2 * (b % 32))
    nonplus = used[None, :] & (cls != 3)
    tc = nonplus.sum(axis=0).astype(np.int32)
    t1 = np.where(tc > 0, nonplus.argmax(axis=0), -1).astype(np.int32)
    anym = (cls == 1).any(axis=1).astype(np.int32)
    return words, tc, t1, anym


def check_both_entry_points(G, X, used, ideal, H):
    words_e, tc_e, t1_e, anym_e = expected(X, used, ideal, H)
    words, anym, _ = G.classify_batch(H)
    words_t, tc, t1 = G.classify_batch_touch(H)
    for got in (words, words_t):
        assert np.array_equal(got[:, used], words_e[:, used]), "class words of live slots"
        assert not got[:, ~used].any(), "class words of dead slots must be zero"
    assert np.array_equal(anym, anym_e)
    assert np.array_equal(tc[used], tc_e[used]) and np.array_equal(t1[used], t1_e[used])
    assert not tc[~used].any() and (t1[~used] == -1).all(), "dead slots must read tc == 0, t1 == -1"
    return tc


def assert_slot_layout(used, ideal):
    nv = len(used)
    assert nv > 128
    full = used[:nv // 64 * 64].reshape(-1, 64)
    assert (~full).all(axis=1).any(), "no aligned run of 64 dead slots"
    assert (full.any(axis=1) & (~full).any(axis=1)).any(), "no run of 64 slots that mixes live and dead"
    assert (used & ideal).any(), "no live ideal direction"
    assert (used & ~ideal).sum() > 8


@pytest.mark.parametrize("B", [32, 33, 1])
def test_live_slots_exact_dead_slots_untouched(B):
    G = PolyEngine(Q)
    build(G)
    X, used, ideal = primal(G)
    assert_slot_layout(used, ideal)
    H = halfspaces(X, used, ideal, B)
    words_e, tc_e, _, anym_e = expected(X, used, ideal, H)
    assert (tc_e[used] > 0).any() and (tc_e[used] < B).any() and anym_e.any()      # (both classes occur)
    check_both_entry_points(G, X, used, ideal, H)
    G.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_slots_killed_after_a_classification_read_untouched(mode):
    """a batch of cuts (one at a time after the batched prefilter: mode 0; in chunks and rounds: mode 1) kills elements that
    the previous classification counted as touched: their counts must not survive"""
    G = PolyEngine(Q)
    G.set_batch_mode(mode)
    more = build(G)
    X, used, ideal = primal(G)
    assert_slot_layout(used, ideal)
    cuts = np.hstack([more, -np.ones((len(more), 1))])            # the halfspaces d.y >= -1 of the cuts to come
    H = halfspaces(X, used, ideal, 33, first=cuts)
    tc0 = check_both_entry_points(G, X, used, ideal, H)
    rc = G.add_cuts(more)
    assert (np.asarray(rc) == 0).any()
    X1, used1, ideal1 = primal(G)
    nv0 = len(used)
    killed = used & ~used1[:nv0]
    assert (killed & (tc0 > 0)).any(), "no element with a touch count was removed"
    assert (used1 & ideal1).any() and len(used1) > nv0
    H1 = halfspaces(X1, used1, ideal1, 33, seed=8)
    check_both_entry_points(G, X1, used1, ideal1, H1)
    G.close()


def test_live_list_over_several_workgroups():
    """more slots than one wave, one workgroup of the list kernel (2048 slots) and one workgroup of the classification cover"""
    G = PolyEngine(Q)
    ph.run_sequence(G, ph.tangent_halfspaces(Q, 800, 11), init_after=Q + 1)
    X, used, ideal = primal(G)
    assert len(used) > 2 * 2048 and used.sum() > 2 * 256 and (~used).sum() > 2048
    check_both_entry_points(G, X, used, ideal, halfspaces(X, used, ideal, 70))
    G.close()
