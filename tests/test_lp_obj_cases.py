"""No GPU: the objective sets of tests/lp_cases.py (what tests/test_lp_obj_general_gpu.py feeds the engine) at the small shapes --
the rules the cost vectors are built by, the folding of the cost on row variables onto the columns, the agreement of the two CPU
yardsticks and the conditions on the inputs -- and that the general sets are still, bit for bit, what they were before the objective
sets got seeds of their own.  `python tests/lp_cases.py obj` makes the same check of the yardsticks for every shape."""
import hashlib

import numpy as np
import pytest

import lp_cases as lc
from lp_cases import NLP, OPTIMAL, UNBOUNDED

SMALL = [(15, 16), (16, 17), (31, 64), (32, 65)]


def test_general_sets_are_what_they_were():
    """the digest was taken from lp_cases.py as it stood before OBJECTIVE_SEEDS: no existing set moved"""
    assert not set(lc.GENERAL_SEEDS) & set(lc.OBJECTIVE_SEEDS)
    h = hashlib.sha256()
    for M, N in lc.GENERAL_SEEDS:
        for arr in ("a", "b"):
            s = lc.general_set(M, N, arr)
            for k in ("A", "cost", "lo", "up", "x0", "vlo", "vup", "perm"):
                h.update(np.ascontiguousarray(s[k]).tobytes())
            h.update(("%d %d" % (s["var_first"], s["var_cnt"])).encode())
    assert h.hexdigest() == "585f56b85a01c4c60381906e3250b63867a13e3fd966aa971d7a97edc41dfb5b"


def test_every_shape_of_the_objective_sets_has_a_seed():
    for M, N in lc.OBJ_SHAPES:
        assert lc.model_seed(M, N) > 0
    seeds = [lc.model_seed(M, N) for M, N in lc.OBJ_SHAPES]
    assert len(set(seeds)) == len(seeds)


@pytest.mark.parametrize("rng_name", lc.OBJ_RANGES)
@pytest.mark.parametrize("M,N", SMALL + [(24, 513)])
def test_cost_vectors_follow_the_rules(M, N, rng_name):
    s = lc.objective_set(M, N, rng_name)
    first, cnt = s["cost_first"], s["cost_cnt"]
    assert (first, cnt) == {"cols": (M, N), "straddle": (M - 3, 8), "head": (M + 1, 5)}[rng_name]
    assert not s["cost"].any() and s["cost"].shape == (N + 1,)
    lo, up = s["lo"][first:first + cnt], s["up"][first:first + cnt]
    flo, fup = np.isfinite(lo), np.isfinite(up)
    c1, c2, c3 = (s["costs"][g] for g in lc.GENS)
    for c in (c1, c2, c3):
        assert c.shape == (NLP, cnt)
        assert not c[:, ~flo & ~fup].any()                   # f
        assert np.all(c[:, flo & ~fup] >= 0)                 # l
        assert np.all(c[:, ~flo & fup] <= 0)                 # u
    assert np.array_equal(c1, np.round(c1))
    if cnt >= N:                # (a range of 5 or 8 variables can be all zero by chance)
        assert c1.any(axis=1).all()
        dense = np.mean(c1[[t for t in range(NLP) if t % 4 != 3]] == 0.0)
        assert np.mean(c1[3::4] == 0.0) > dense + 0.25, (np.mean(c1[3::4] == 0.0), dense)      # every fourth vector: 70 % of what is left zeroed
    ratio = np.divide(c2, c1[s["perm"]], out=np.ones_like(c2), where=c1[s["perm"]] != 0)
    assert np.all((ratio >= 0.9) & (ratio <= 1.1)) and np.array_equal(c2 == 0, c1[s["perm"]] == 0)
    ratio = np.divide(c3, c2, out=np.ones_like(c3), where=c2 != 0)
    assert np.all((ratio >= 0.95) & (ratio <= 1.05)) and np.array_equal(c3 == 0, c2 == 0)
    assert sorted(s["perm"]) == list(range(NLP)) and not np.any(s["perm"] == np.arange(NLP))
    # the folded cost is the same function on r = A x
    rng = np.random.default_rng(1)
    for g in lc.GENS:
        for t in (0, 3, NLP - 1):
            x = rng.normal(size=N)
            full = np.concatenate([s["A"] @ x, x])
            f = s["folded"][g][t]
            assert f.shape == (N + 1,) and f[0] == 0.0
            np.testing.assert_allclose(f[1:] @ x, s["costs"][g][t] @ full[first:first + cnt], rtol=1e-12, atol=1e-12)
    if rng_name == "straddle":
        assert first < M < first + cnt and any(s["costs"]["gen1"][:, :M - first].any(axis=0))      # some row variable carries a cost


@pytest.mark.parametrize("rng_name", lc.OBJ_RANGES)
@pytest.mark.parametrize("M,N", SMALL)
def test_yardsticks_agree_on_an_objective_set(oracle, M, N, rng_name):
    ref, w, n = lc.assert_objective_references_agree(M, N, rng_name)
    assert all(r["st"] == r["st_highs"] == OPTIMAL for g in lc.GENS for r in ref[g])
    assert n["boxed_at_up"] > 0 and n["boxed_at_lo"] > 0
    if rng_name == "cols":
        assert 4 * n["nonbasic"] >= n["carrying"] > 0
    assert w["gap"] <= 1e-9


@pytest.mark.parametrize("M,N", SMALL)
def test_yardsticks_agree_on_the_unbounded_objectives(oracle, M, N):
    s = lc.unbounded_objective_set(M, N)
    assert (s["cost_first"], s["cost_cnt"]) == (M, 3) and not s["A"][:, 0].any()
    assert [tuple(s["costs"][t]) for t in (2, 9, 5)] == [(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)]
    assert not s["costs"][[t for t in range(NLP) if t not in lc.UNB_LPS], 0].any()
    rows, _ = lc.unbounded_objective_references(M, N)
    assert [r["st"] for r in rows] == [UNBOUNDED if t in (2, 5, 9) else OPTIMAL for t in range(NLP)]
    assert [r["st_highs"] for r in rows] == [r["st"] for r in rows]
