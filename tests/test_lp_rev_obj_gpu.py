"""GPU: batches of LPs that differ in their objective (bslv_lpq_solve_batch_obj) in the REVISED form of the LP engine.

The model is P1(w) exactly as the dual variant of Benson's algorithm builds it (dual_benson, vlp_phases.hip): rows [A 0; -P I],
zero engine cost, the weights w as the cost of the q columns y.  min w.y  s.t.  A x >= 1, -P x + y = 0, x >= 0, y free.
BSLV_LP_REV=1 forces the revised form (basis inverse per LP, the new reduced-cost row formed by k_rev_price), 0 the tableau
form.  The same chain of solves runs through both: the feasibility LP in slot 0, an in-place solve there (PART 1 of
dual_benson), a batch of weights from slot 0 into new slots, a second generation with perturbed weights from those slots, and an
in-place batch on the second generation."""
import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.lp import LpEngine, bounds_from_types

pytestmark = pytest.mark.gpu
RTOL = 1e-9
OPTIMAL, UNBOUNDED = 4, 1


def _sparse_covering(m, n, q, seed, per_col=4, dense_cols=0):
    """covering VLP with a sparse A (per_col non-zeros per column, every row hit) and sparse objectives; dense_cols columns with
    m / 2 non-zeros (the generator of test_lp_gpu.py, except that every column of P has a non-zero: P1(w) is then not solved by
    the basis of P1(w') for every other w')"""
    rng = np.random.default_rng(seed)
    prob = synth.covering_vlp(m, n, q, seed)
    A = np.zeros((m, n))
    for j in range(n):
        k = m // 2 if j < dense_cols else per_col
        rows = rng.choice(m, size=k, replace=False)
        A[rows, j] = rng.uniform(0.5, 1.5, size=k) * (0.2 if j < dense_cols else 1.0)
    for i in range(m):
        if not A[i].any():
            A[i, rng.integers(n)] = 1.0
    mask = rng.random((q, n)) < 0.3
    mask[rng.integers(q, size=n), np.arange(n)] = True      # (a column of P without a non-zero would make y = 0 optimal for every w >= 0)
    P = prob["P"] * mask
    P[:, 0] = prob["P"][:, 0]
    return dict(prob, A=A, P=P)


class P1Model:
    """P1(w) of dual_benson (hom = 0): M = m + q rows, N = n + q columns, variable ids 0..M-1 rows, M.. columns"""

    def __init__(self, prob):
        m, n, q = prob["m"], prob["n"], prob["q"]
        M, N = m + q, n + q
        L = np.zeros((M, N))
        L[:m, :n] = prob["A"]
        L[m:, :n] = -prob["P"]
        L[m:, n:] = np.eye(q)
        rlo, rup = bounds_from_types(prob["rtype"], prob["rlb"], prob["rub"])
        clo, cup = bounds_from_types(prob["ctype"], prob["clb"], prob["cub"])
        self.lo = np.concatenate([rlo, np.zeros(q), clo, np.full(q, -np.inf)])
        self.up = np.concatenate([rup, np.zeros(q), cup, np.full(q, np.inf)])
        self.m, self.n, self.q, self.M, self.N, self.L = m, n, q, M, N, L
        self.y_first = M + n          # cost range of solve_batch_obj, primal values of y

    def engine(self, slots):
        return LpEngine(self.M, self.N, self.L, self.lo, self.up, np.zeros(self.N + 1), 0, 0, slots)


def _weights(rng, B, q):
    W = rng.uniform(0.1, 1.0, size=(B, q))
    return W / W.sum(axis=1, keepdims=True)


def _oracle_obj(model, W):
    import oracle_api
    out = np.empty(len(W))
    for b, w in enumerate(W):
        cost = np.zeros(model.N + 1)
        cost[1 + model.n:] = w
        olp = oracle_api.OracleLP(model.L, model.lo, model.up, cost)      # (a new LP each time: solved from scratch)
        assert olp.solve(1) == OPTIMAL
        out[b] = olp.obj()
        olp.close()
    return out


def _check_certificates(model, prob, eng, slots, W, obj):
    """y = P x, x feasible; the duals -s reads (rows) and the reduced costs (columns) have the signs their bounds allow, sit only
    on variables at a bound, and give the objective back: strong duality"""
    M, N, n, q = model.M, model.N, model.n, model.q
    val = eng.primal(slots, 0, M + N)
    dual = eng.dual(slots, 0, M + N)
    x, y = val[:, M:M + n], val[:, model.y_first:]
    np.testing.assert_allclose(x @ prob["P"].T, y, rtol=0, atol=1e-8)
    assert np.all(x >= -1e-9) and np.all(x @ prob["A"].T >= 1 - 1e-8)
    np.testing.assert_allclose(np.einsum("bk,bk->b", W, y), obj, rtol=1e-9, atol=1e-9)
    lo, up = model.lo[None, :], model.up[None, :]
    at_lo = np.abs(val - lo) <= 1e-8 * (1 + np.abs(np.where(np.isinf(lo), 0, lo)))
    at_up = np.abs(val - up) <= 1e-8 * (1 + np.abs(np.where(np.isinf(up), 0, up)))
    fixed = (lo == up) & np.ones_like(val, bool)
    tol = 1e-9
    assert np.all(fixed | (dual <= tol) | at_lo), "positive dual on a variable off its lower bound"
    assert np.all(fixed | (dual >= -tol) | at_up), "negative dual on a variable off its upper bound"
    bound = np.where(dual > 0, np.broadcast_to(lo, val.shape), np.broadcast_to(up, val.shape))
    bound = np.where(fixed, np.broadcast_to(lo, val.shape), bound)
    bound = np.where(np.abs(dual) <= 1e-12, 0.0, bound)
    assert np.all(np.isfinite(bound))
    np.testing.assert_allclose((dual * bound).sum(axis=1), obj, rtol=1e-8, atol=1e-8)
    return dual[:, :model.m]


CASES = [(40, 300, 3, 5, 16, 0), (90, 700, 4, 9, 24, 0), (120, 6000, 3, 11, 8, 6)]


def _chain(monkeypatch, model, rev, B, seed, extra_env=()):
    monkeypatch.setenv("BSLV_LP_REV", rev)
    for k, v in extra_env:
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(seed)
    q = model.q
    w0 = np.full((1, q), 1.0 / q)
    W1 = _weights(rng, B, q)
    W2 = np.abs(W1 * rng.uniform(0.9, 1.1, size=W1.shape))
    W2 /= W2.sum(axis=1, keepdims=True)
    W3 = np.abs(W2 * rng.uniform(0.95, 1.05, size=W2.shape))
    W3 /= W3.sum(axis=1, keepdims=True)
    eng = model.engine(2 * B + 1)
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(rev)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))        # the feasibility LP (zero objective)
    assert st[0] == OPTIMAL, st
    st, _ = eng.solve_batch_obj([0], [0], model.y_first, w0)                       # in place (PART 1 of dual_benson)
    assert st[0] == OPTIMAL, st
    out = dict(obj0=eng.obj([0]).copy())
    src = np.zeros(B, np.int32)
    dst = np.arange(1, B + 1, dtype=np.int32)
    st, it = eng.solve_batch_obj(src, dst, model.y_first, W1)
    assert np.all(st == OPTIMAL), (rev, st)
    out.update(obj1=eng.obj(dst).copy(), it1=int(it.sum()))
    dst2 = np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    st, it = eng.solve_batch_obj(dst, dst2, model.y_first, W2)                     # warm starts from the children
    assert np.all(st == OPTIMAL), (rev, st)
    out.update(obj2=eng.obj(dst2).copy(), it2=int(it.sum()))
    st, it = eng.solve_batch_obj(dst2, dst2, model.y_first, W3)                    # in place
    assert np.all(st == OPTIMAL), (rev, st)
    out.update(obj3=eng.obj(dst2).copy())
    out.update(W=(w0, W1, W2, W3), dst=dst, dst2=dst2)
    return eng, out


@pytest.mark.parametrize("m,n,q,seed,B,dense_cols", CASES)
def test_objective_batches_in_the_revised_form(monkeypatch, oracle, m, n, q, seed, B, dense_cols):
    """statuses, optimal values against the tableau form and against the oracle LP solved from scratch (1e-9), y = P x, feasible x,
    signs of the duals and strong duality, in the revised form.  The third case has rows of 6000 columns and six columns of 60
    non-zeros: k_rev_price runs on 12 slices per LP and the dense columns go to rev_row_slice's queue (a wave per column)."""
    prob = _sparse_covering(m, n, q, seed, dense_cols=dense_cols)
    model = P1Model(prob)
    res = {}
    for rev in ("0", "1"):
        eng, out = _chain(monkeypatch, model, rev, B, seed)
        if rev == "1":
            w0, W1, W2, W3 = out["W"]
            for slots, W, obj in ((np.array([0], np.int32), w0, out["obj0"]), (out["dst"], W1, out["obj1"]), (out["dst2"], W3, out["obj3"])):
                u = _check_certificates(model, prob, eng, slots, W, obj)
                assert np.all(u >= -1e-9)                                          # -s: u >= 0 on the cover rows
        eng.close()
        res[rev] = out
    a, b = res["0"], res["1"]
    assert b["it1"] > 0 and b["it2"] >= 0
    for k in ("obj0", "obj1", "obj2", "obj3"):
        np.testing.assert_allclose(b[k], a[k], rtol=RTOL, atol=1e-9, err_msg=k)
    w0, W1, W2, W3 = b["W"]
    for k, W in (("obj0", w0), ("obj1", W1), ("obj2", W2), ("obj3", W3)):
        np.testing.assert_allclose(b[k], _oracle_obj(model, W), rtol=RTOL, atol=1e-9, err_msg=k)


def test_objective_batches_with_the_price_vector_in_global_memory(monkeypatch):
    """y of k_rev_price from global scratch (k_rev_y), as for M beyond what LDS holds: the same values as with y in LDS"""
    prob = _sparse_covering(120, 6000, 3, 11, dense_cols=6)
    model = P1Model(prob)
    res = {}
    for lds in ("1", "0"):
        eng, out = _chain(monkeypatch, model, "1", 8, 11, extra_env=(("BSLV_REV_PRICE_LDS", lds),))
        eng.close()
        res[lds] = out
    for k in ("obj0", "obj1", "obj2", "obj3"):
        assert np.array_equal(res["1"][k], res["0"][k]), k


@pytest.mark.parametrize("rev", ["0", "1"])
def test_unbounded_objective_is_reported(monkeypatch, rev):
    """w = -e_0: y_0 = P_0 x grows without bound along x >= 0"""
    monkeypatch.setenv("BSLV_LP_REV", rev)
    prob = _sparse_covering(40, 300, 3, 5)
    model = P1Model(prob)
    eng = model.engine(4)
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
    assert st[0] == OPTIMAL
    W = np.array([[-1.0, 0.0, 0.0], [0.2, 0.3, 0.5]])
    st, _ = eng.solve_batch_obj([0, 0], [1, 2], model.y_first, W)
    assert st[0] == UNBOUNDED and st[1] == OPTIMAL, st
    eng.close()


def test_non_zero_engine_cost_is_still_refused(monkeypatch):
    monkeypatch.setenv("BSLV_LP_REV", "1")
    prob = _sparse_covering(40, 300, 3, 5)
    model = P1Model(prob)
    cost = np.zeros(model.N + 1)
    cost[1] = 1.0
    eng = LpEngine(model.M, model.N, model.L, model.lo, model.up, cost, 0, 0, 4)
    assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
    eng.reset_slot(0)
    with pytest.raises(Exception, match="non-zero cost"):
        eng.solve_batch_obj([0], [1], model.y_first, np.full((1, 3), 1.0 / 3))
    eng.close()


def test_undefined_hook_only_sets_the_status(monkeypatch):
    """BSLV_LP_OBJ_UNDEFINED=K:b reports LP b of the K-th objective batch of an engine as UNDEFINED and changes nothing else"""
    prob = _sparse_covering(40, 300, 3, 5)
    model = P1Model(prob)
    W = _weights(np.random.default_rng(3), 4, 3)
    res = {}
    for hook in (None, "1:2"):
        monkeypatch.setenv("BSLV_LP_REV", "1")
        if hook:
            monkeypatch.setenv("BSLV_LP_OBJ_UNDEFINED", hook)
        eng = model.engine(12)
        eng.reset_slot(0)
        eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
        st1, _ = eng.solve_batch_obj(np.zeros(4, np.int32), np.arange(1, 5, dtype=np.int32), model.y_first, W)
        st2, _ = eng.solve_batch_obj(np.zeros(4, np.int32), np.arange(5, 9, dtype=np.int32), model.y_first, W)
        res[hook] = (st1, st2, eng.obj(np.arange(1, 9, dtype=np.int32)))
        eng.close()
    assert list(res[None][0]) == [OPTIMAL] * 4 and list(res[None][1]) == [OPTIMAL] * 4
    assert list(res["1:2"][0]) == [OPTIMAL, OPTIMAL, 3, OPTIMAL] and list(res["1:2"][1]) == [OPTIMAL] * 4
    assert np.array_equal(res[None][2], res["1:2"][2])
