"""k_select_cached (the plain dual selection of the tableau form with a pivot's row and column state kept in registers and LDS) against
k_select<false>, which BSLV_SELECT_CACHE=0 brings back: same pivots, same objective values, duals, y and x bit for bit.

Shapes by where the register path can go wrong (LP rows M = m + 2q + 1, LP columns N = n + q + 1; NT = 256 threads):
  N < NT (threads without a column), NT < N < 2 NT with M < NT (threads without a row), 2 NT < N < 4 NT and N = 6 NT - 1 (the other two
  column counts per thread), M = NT + 1 (one row beyond a stripe), M > 4 NT (a second round of rows per thread), and the launches that
  do not take the new path at all (extended selection, 1024 threads) or that cut the KP selections of a pass into KP launches."""
import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine

pytestmark = pytest.mark.gpu

SWITCHES = ("BSLV_SELECT_CACHE", "BSLV_SELECT_FUSE", "BSLV_SELECT_NT")


def _random_V(model, prob, rng, B):
    n = prob["n"]
    X = rng.random((B, n)) * (3.0 / n) + 1.0 / n
    Y = X @ prob["P"].T
    return Y * rng.uniform(0.2, 1.2, size=(B, 1)) + rng.normal(scale=0.05, size=Y.shape)


def _covering(m, n, q, seed, B):
    prob = synth.covering_vlp(m, n, q, seed)
    model = P2Model(prob)
    return prob, model, _random_V(model, prob, np.random.default_rng(12), B)


def _boxed(B):
    prob = synth.fold_singleton_rows(synth.degenerate_vlp(240, 120, 4, 5))
    model = P2Model(prob)
    rng = np.random.default_rng(12)
    V = rng.random((B, 120)) @ prob["P"].T + rng.normal(scale=0.5, size=(B, 4))
    V[: B // 4] = np.round(V[: B // 4])
    return prob, model, V


CASES = {
    "N=104 M=207": (lambda: _covering(200, 100, 3, 1, 96), {}),
    "N=304 M=67": (lambda: _covering(60, 300, 3, 2, 48), {}),
    "N=704 M=47": (lambda: _covering(40, 700, 3, 3, 16), {}),
    "N=1535 M=37": (lambda: _covering(30, 1531, 3, 4, 8), {}),
    "N=124 M=257": (lambda: _covering(250, 120, 3, 5, 16), {}),
    "N=64 M=1037": (lambda: _covering(1030, 60, 3, 6, 8), {}),
    "extended selection": (lambda: _boxed(48), {}),
    "N=104 M=207 six launches": (lambda: _covering(200, 100, 3, 1, 96), {"BSLV_SELECT_FUSE": "0"}),
    "N=104 M=207 1024 threads": (lambda: _covering(200, 100, 3, 1, 96), {"BSLV_SELECT_NT": "1024"}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_select_cache_is_bit_identical_to_the_plain_selection(monkeypatch, case):
    import oracle_api  # noqa: F401  (same import order as the other tests)
    make, env = CASES[case]
    prob, model, V = make()
    B = len(V)
    ub = model.ub_for(V)
    res = {}
    for cache in ("0", "1"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if cache == "0":
            monkeypatch.setenv("BSLV_SELECT_CACHE", "0")       # (the default is the new path)
        eng = LpEngine.from_model(model, pool_slots=B + 1)
        eng.reset_slot(0)
        st0, it0 = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), ub[:1])
        assert st0[0] == 4
        src = np.zeros(B, np.int32)
        dst = np.arange(1, B + 1, dtype=np.int32)
        st, it = eng.solve_batch(src, dst, np.full((B, model.r), -np.inf), ub)
        assert np.all(st == 4)
        res[cache] = (int(it0[0]), it.copy(), eng.obj(dst).copy(), eng.dual(dst, model.w_first, model.q).copy(),
                      eng.primal(dst, model.y_first, model.q).copy(), eng.primal(dst, model.M, prob["n"]).copy())
        eng.close()
    a, b = res["0"], res["1"]
    print("%s: cold LP %d pivots, batch of %d: %d pivots" % (case, a[0], B, int(a[1].sum())))
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), "pivot counts differ"
    assert a[1].sum() > B, "the batch needs pivots for this to mean anything"
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def _infeasible_lp():
    # x1 + x2 >= 2 and x1 + x2 <= 1, x >= 0, min x1 + x2: the second row finds no entering candidate
    A = np.array([[1.0, 1.0], [1.0, 1.0]])
    lo = np.array([2.0, -np.inf, 0.0, 0.0])
    up = np.array([np.inf, 1.0, np.inf, np.inf])
    return A, lo, up, np.array([0.0, 1.0, 1.0]), 0


def _unbounded_lp():
    # min -x1 with x1 free above (the second LP of test_lp_gpu.test_infeasible_and_unbounded_status): optimal on an artificial bound
    A = np.array([[1.0, 1.0]])
    lo = np.array([-np.inf, 0.0, 0.0])
    up = np.array([np.inf, np.inf, np.inf])
    return A, lo, up, np.array([0.0, -1.0, 0.0]), 1


@pytest.mark.parametrize("make", [_infeasible_lp, _unbounded_lp])
def test_select_cache_ends_infeasible_and_unbounded_lps_as_the_plain_selection(monkeypatch, make):
    """The cases above all end OPTIMAL.  Two LPs without a boxed variable (no variable has two finite bounds, so the plain dual
    selection runs and k_select_cached takes it) that end the other ways: no entering candidate for a violated row (INFEASIBLE, 0) and an
    active artificial bound at the optimum of the bounded problem (UNBOUNDED, 1).  Same status and same pivot count through both
    kernels, and the status of the CPU oracle."""
    import oracle_api
    A, lo, up, cost, expected = make()
    M, N = A.shape
    olp = oracle_api.OracleLP(A, lo, up, cost)
    ost = olp.solve(1)
    olp.close()
    assert ost == expected
    res = {}
    for cache in ("0", "1"):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if cache == "0":
            monkeypatch.setenv("BSLV_SELECT_CACHE", "0")
        eng = LpEngine(M, N, A, lo, up, cost, 0, 0, 2)
        eng.reset_slot(0)
        st, it = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
        stats = eng.last_stats()
        eng.close()
        print("%s cache %s: status %d, %d pivots, %s" % (make.__name__, cache, st[0], it[0], stats))
        assert stats["perturbations"] == 0 and stats["flip_iterations"] == 0 and stats["primal_steps"] == 0      # (not the extended selection)
        res[cache] = (int(st[0]), int(it[0]))
    assert res["0"][0] == expected and res["1"][0] == expected
    assert res["0"] == res["1"], "status or pivot count differs"
