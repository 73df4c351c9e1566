"""k_init_grouped (the start of a batch whose LPs share parents: a parent's tableau rows are read once into registers for a chunk of its
children) against k_init, which BSLV_INIT_GROUP=0 brings back: same statuses, pivots, objective values, duals, y and x bit for bit.

One cold LP in slot 0, P parents solved from it into slots 1..P with different V, then a batch of B children whose parents are
INTERLEAVED in the batch, with families of unequal size.  Shapes by where the grouping can go wrong (LP rows M = m + 2q + 1, LP
columns N = n + q + 1, rows of ld = N rounded up to 16 doubles; a lane holds EPL double2 of a row, a wave R rows, a workgroup 4 R):
  ld/2 = 56 (lanes without a column, EPL 1), 104 (EPL 2), 152 (EPL 4, the last of a lane's entries only in some lanes), 352 (EPL 8,
  R 4), 752 (EPL 16, R 2) and 1056 (no instance: k_init); M + 1 = 28 (less than a workgroup's rows), 33 (row M alone in the second
  workgroup, first row of a wave), 68, 108 and 208 (not a multiple of 32); every family of size 1, one family of 48 (cut into chunks of 4
  children), five unequal families; children with their parent's V (no pivot: what they return is the start's beta untouched) among
  children that pivot; a batch in place; the revised form; a batch of new objectives (k_init's by design)."""
import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine, bounds_from_types

pytestmark = pytest.mark.gpu

OPTIMAL = 4


def _random_V(prob, rng, B):
    n = prob["n"]
    X = rng.random((B, n)) * (3.0 / n) + 1.0 / n
    Y = X @ prob["P"].T
    return Y * rng.uniform(0.2, 1.2, size=(B, 1)) + rng.normal(scale=0.05, size=Y.shape)


def _families(P, B, rng):
    """parent (0-based) of each child: P = B one child each, else unequal families (about half of the batch in the first), shuffled"""
    if P == B:
        return rng.permutation(B)
    w = 0.5 ** np.arange(1, P + 1)
    w[-1] *= 2
    sizes = np.maximum(1, np.floor(w * B).astype(int))
    sizes[0] += B - sizes.sum()
    return rng.permutation(np.repeat(np.arange(P), sizes))


# m, n, q, seed, P, B, expected kernel ("grouped" / "init"), environment, also a batch in place
CASES = {
    "ld2=56 M+1=208 five families": (200, 100, 3, 1, 5, 48, "grouped", {}, True),
    "ld2=56 M+1=208 one family": (200, 100, 3, 1, 1, 48, "grouped", {}, False),
    "ld2=56 M+1=208 families of one": (200, 100, 3, 1, 16, 16, "grouped", {}, False),
    "ld2=56 M+1=28": (20, 100, 3, 7, 3, 24, "grouped", {}, False),
    "ld2=104 M+1=33": (25, 200, 3, 8, 3, 24, "grouped", {}, True),
    "ld2=152 M+1=68": (60, 300, 3, 2, 4, 32, "grouped", {}, False),
    "ld2=352 M+1=41": (33, 700, 3, 3, 3, 16, "grouped", {}, False),
    "ld2=352 M+1=33": (25, 700, 3, 3, 3, 16, "grouped", {}, False),
    "ld2=752 M+1=37": (29, 1500, 3, 4, 2, 12, "grouped", {}, False),
    "ld2=1056 M+1=108 k_init": (100, 2100, 3, 9, 2, 12, "init", {}, False),
    "revised form": (40, 300, 3, 5, 2, 16, "grouped", {"BSLV_LP_REV": "1"}, False),
}


def _run(monkeypatch, group, make_prob, P, B, env, in_place):
    monkeypatch.delenv("BSLV_INIT_GROUP", raising=False)
    monkeypatch.delenv("BSLV_LP_REV", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not group:
        monkeypatch.setenv("BSLV_INIT_GROUP", "0")       # (the default is the new kernel)
    prob = make_prob()
    model = P2Model(prob)
    rng = np.random.default_rng(12)
    VP = _random_V(prob, rng, P)
    fam = _families(P, B, rng)
    V = _random_V(prob, rng, B)
    still = np.arange(B) % 5 == 2                                  # every fifth child: its parent's V, no pivot
    V[still] = VP[fam[still]]
    V2 = V * 1.07 + 0.01
    free = lambda k: np.full((k, model.r), -np.inf)
    eng = LpEngine.from_model(model, pool_slots=P + B + 1)
    eng.reset_slot(0)
    st0, it0 = eng.solve_batch([0], [0], free(1), model.ub_for(VP[:1]))
    assert st0[0] == OPTIMAL
    par = np.arange(1, P + 1, dtype=np.int32)
    stp, itp = eng.solve_batch(np.zeros(P, np.int32), par, free(P), model.ub_for(VP))
    assert np.all(stp == OPTIMAL)
    chunks = [eng.last_stats()["init_chunks"]]
    src = par[fam]
    dst = np.arange(P + 1, P + B + 1, dtype=np.int32)
    st, it = eng.solve_batch(src, dst, free(B), model.ub_for(V))
    assert np.all(st == OPTIMAL)
    chunks.append(eng.last_stats()["init_chunks"])
    get = lambda s: [eng.obj(s).copy(), eng.dual(s, model.w_first, model.q).copy(), eng.primal(s, model.y_first, model.q).copy(), eng.primal(s, model.M, prob["n"]).copy()]
    out = dict(ints=[st0, it0, stp, itp, st, it], vals=get(par) + get(dst), pivots=int(it.sum()), still=it[still].copy(), chunks=chunks, fam=fam)
    if in_place:
        st2, it2 = eng.solve_batch(dst, dst, free(B), model.ub_for(V2))
        assert np.all(st2 == OPTIMAL)
        out["ints"] += [st2, it2]
        out["vals"] += get(dst)
        out["chunks"].append(eng.last_stats()["init_chunks"])
    eng.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_grouped_start_is_bit_identical_to_k_init(monkeypatch, case):
    import oracle_api  # noqa: F401  (same import order as the other tests)
    m, n, q, seed, P, B, kernel, env, in_place = CASES[case]
    if "BSLV_LP_REV" in env:
        from test_lp_gpu import _sparse_covering
        make = lambda: _sparse_covering(m, n, q, seed)
    else:
        make = lambda: synth.covering_vlp(m, n, q, seed)
    a = _run(monkeypatch, False, make, P, B, env, in_place)
    b = _run(monkeypatch, True, make, P, B, env, in_place)
    print("%s: batch of %d from %d parents: %d pivots, %d children without one; chunks %s / %s" % (case, B, P, a["pivots"], int((a["still"] == 0).sum()), a["chunks"], b["chunks"]))
    assert all(c == 0 for c in a["chunks"]), "BSLV_INIT_GROUP=0 must run k_init"
    if kernel == "init":
        assert all(c == 0 for c in b["chunks"]), "rows beyond the widest instance must run k_init"
    else:
        # chunks of 4 children at these sizes: the parents' batch is one family of P, the children's is cut per family, in place every LP is its own parent
        fam = np.bincount(a["fam"])
        expect = [-(-P // 4), int(sum(-(-int(f) // 4) for f in fam if f))] + ([B] if in_place else [])
        assert b["chunks"] == expect, (b["chunks"], expect)
    assert a["pivots"] > B, "the batch needs pivots for this to mean anything"
    assert np.any(a["still"] == 0), "some children must end without a pivot: their values are the start's beta"
    for x, y in zip(a["ints"], b["ints"]):
        assert np.array_equal(x, y), "statuses or pivot counts differ"
    for x, y in zip(a["vals"], b["vals"]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_new_objectives_start_with_k_init_and_agree(monkeypatch):
    """solve_batch_obj in the tableau form: k_prep writes each child's reduced-cost row into the child's own slot, so these batches keep
    k_init whatever the switch says; same results bit for bit, two parents."""
    import oracle_api  # noqa: F401
    monkeypatch.setenv("BSLV_LP_REV", "0")
    prob = synth.covering_vlp(40, 120, 3, 5)
    m, n, q = prob["m"], prob["n"], prob["q"]
    M, N = m + q, n + q
    L = np.zeros((M, N))
    L[:m, :n] = prob["A"]
    L[m:, :n] = -prob["P"]
    L[m:, n:] = np.eye(q)
    rlo, rup = bounds_from_types(prob["rtype"], prob["rlb"], prob["rub"])
    clo, cup = bounds_from_types(prob["ctype"], prob["clb"], prob["cub"])
    lo = np.concatenate([rlo, np.zeros(q), clo, np.full(q, -np.inf)])
    up = np.concatenate([rup, np.zeros(q), cup, np.full(q, np.inf)])
    rng = np.random.default_rng(3)
    B = 16
    W = rng.uniform(0.1, 1.0, size=(2 + B, q))
    W /= W.sum(axis=1, keepdims=True)
    src = np.array([1, 2, 2, 1, 2, 2, 2, 1, 2, 2, 1, 2, 2, 2, 2, 2], np.int32)
    dst = np.arange(3, 3 + B, dtype=np.int32)
    res = {}
    for group in ("0", "1"):
        monkeypatch.setenv("BSLV_INIT_GROUP", group)
        eng = LpEngine(M, N, L, lo, up, np.zeros(N + 1), 0, 0, B + 3)
        eng.reset_slot(0)
        st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))        # the feasibility LP (zero objective)
        assert st[0] == OPTIMAL
        stp, itp = eng.solve_batch_obj([0, 0], [1, 2], M + n, W[:2])
        assert np.all(stp == OPTIMAL)
        st, it = eng.solve_batch_obj(src, dst, M + n, W[2:])
        assert np.all(st == OPTIMAL)
        assert eng.last_stats()["init_chunks"] == 0
        res[group] = (itp, it, eng.obj(dst).copy(), eng.dual(dst, 0, M + N).copy(), eng.primal(dst, 0, M + N).copy())
        eng.close()
    a, b = res["0"], res["1"]
    assert a[1].sum() > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
