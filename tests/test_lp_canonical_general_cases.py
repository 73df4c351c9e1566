"""No GPU: the tied general sets of tests/canonical_general_cases.py (what tests/test_lp_canonical_general_gpu.py feeds the engine)
-- the rules the ties and the directions are made by, the keep rule restated on the kept cases, the conditions on every set and on the
required sets together, and that HiGHS calls the shifted LP of every LP of the exit sets infeasible; and the wide P2 sets of
tests/canonical_cases.py (WIDE) against check_case_set.  `python tests/canonical_general_cases.py` and `python
tests/canonical_cases.py` print the same tables."""
import numpy as np
import pytest

import canonical_cases as cc
import canonical_general_cases as cg
import lp_cases as lc
from bensolve_amd.lp import P2Model
from lp_cases import OPTIMAL, INFEASIBLE, NLP


@pytest.mark.parametrize("arr", ["a", "b"])
@pytest.mark.parametrize("M,N", cg.SHAPES)
def test_tied_set_meets_its_conditions(oracle, M, N, arr):
    c = cg.tied_set(M, N, arr)
    print(cg.table_line(c))
    cg.check_tied_set(c)
    s = lc.general_set(M, N, arr)
    ref, _ = lc.assert_references_agree(M, N, arr)
    first, cnt = c["var_first"], c["var_cnt"]
    assert c["candidates"] == sum(r["st"] == r["st_highs"] == OPTIMAL for r in ref) and len(c["lps"]) + c["dropped"] == c["candidates"]
    # the directions
    d = np.array([1.0 + cc.hash01(k) for k in range(cnt)])
    assert np.array_equal(c["dir"], d if arr == "a" else d * np.where(np.arange(cnt) % 2, -1.0, 1.0))
    for b, t in enumerate(c["lps"]):
        lo0, up0 = s["lps"][t]
        lo, up = c["bounds"][b]
        ties = c["ties"][b]
        # a tie moves one finite bound of a per-LP variable that was strictly inside onto its value; nothing else moves
        assert 1 <= len(ties) <= cg.TIES
        moved = np.nonzero((lo != lo0) | (up != up0))[0]
        assert sorted(moved) == sorted(k for k, _ in ties) and all(first <= k < first + cnt for k in moved)
        assert np.array_equal(np.isfinite(lo), np.isfinite(s["lo"])) and np.array_equal(np.isfinite(up), np.isfinite(s["up"]))
        for k, side in ties:
            assert lo0[k] < up0[k] and lo0[k] + cg.INSIDE <= c["prim"][b][k] <= up0[k] - cg.INSIDE
            assert (lo[k], up[k]) == ((c["prim"][b][k], up0[k]) if side == "lo" else (lo0[k], c["prim"][b][k]))
        assert np.array_equal(c["vlo"][b], lo[first:first + cnt]) and np.array_equal(c["vup"][b], up[first:first + cnt])
        # the optimum is what it was
        np.testing.assert_allclose(c["z"][b], ref[t]["obj"], rtol=lc.RTOL, atol=1e-9)
        st, z, _, _ = cg.solve_rowform(c["A"], lo, up, c["cost"])
        assert st == OPTIMAL
        np.testing.assert_allclose(z, c["z"][b], rtol=lc.RTOL, atol=1e-9)
        # the expected dual is optimal at t = 0, in lc.certify's signs
        cert = lc.certify(c["A"], lo, up, c["cost"], OPTIMAL, c["z"][b], c["prim"][b], c["dual"][b])
        lc.assert_certified(cert, c["z"][b], 0.0, (M, N, arr, t))
        assert c["degenerate"][b] == any(abs(c["dual"][b][k]) > cg.DEGENERATE for k, _ in ties)


def test_keep_rule_on_one_set(oracle):
    """the keep rule restated from outside: the expected dual is the dual at T1 and at T2, and the value is linear through 0"""
    c = cg.tied_set(16, 17, "b")
    for b in range(len(c["lps"])):
        lo, up = c["bounds"][b]
        z = []
        for t in (cc.T1, cc.T2):
            st, zt, _, y = cg.solve_rowform(c["A"], *cg.shifted(lo, up, c["var_first"], c["dir"], t), c["cost"])
            assert st == OPTIMAL and np.abs(y - c["dual"][b]).max() <= cc.SAME_W
            z.append(zt)
        assert abs((z[0] - c["z"][b]) - 2.0 * (z[1] - c["z"][b])) <= cc.OPT_TOL * (1.0 + abs(c["z"][b]))
        # ... and its slope is the one the expected dual gives: the sum of dual times the direction over the shifted bounds
        k = slice(c["var_first"], c["var_first"] + c["var_cnt"])
        np.testing.assert_allclose((z[0] - z[1]) / (cc.T1 - cc.T2), c["dual"][b][k] @ c["dir"], rtol=1e-6, atol=1e-6)


def test_required_sets_together_hold_every_kind_of_tie(oracle):
    sets = [cg.tied_set(M, N, arr) for M, N in cg.REQUIRED for arr in ("a", "b")]
    tot = cg.check_all_sets(sets)
    print("required sets together: %s" % tot)
    assert tot["lower"] > 0 and tot["upper"] > 0 and tot["boxed_col"] > 0


@pytest.mark.parametrize("M,N", cg.EXIT_SHAPES)
def test_shifted_lps_of_the_exit_sets_are_infeasible(oracle, M, N):
    e = cg.exit_set(M, N)
    ref, _ = lc.assert_references_agree(M, N, "a")
    assert list(e["lps"]) == [t for t in range(NLP) if ref[t]["st"] == OPTIMAL] and len(e["lps"]) >= 12
    print("canonical_general_cases exit M %d N %d: %d OPTIMAL LPs, shifted statuses %s" % (M, N, len(e["lps"]), e["shifted_status"]))
    assert all(st == (INFEASIBLE, INFEASIBLE) for st in e["shifted_status"]), e["shifted_status"]
    d = e["dir"]
    assert np.all(d[0::2] >= 1.0) and np.all(d[1::2] <= -1.0) and len(d) == M


@pytest.mark.parametrize("N", sorted(cc.WIDE))
def test_wide_p2_set_meets_its_conditions(N):
    """the number of columns the name promises, and the unchanged conditions of canonical_cases.check_case_set"""
    name = cc.WIDE_NAMES[N]
    prob, c = cc.cases(name)
    model = P2Model(prob)
    print("canonical_cases %s: P2 %d x %d, candidates %d kept %d degenerate %d dropped %d" % (
        name, model.M, model.N, c["candidates"], len(c["V"]), int(c["degenerate"].sum()), c["dropped"]))
    assert model.N == N and model.M + 1 == (32 if prob["q"] == 3 else 34) and prob["m"] == 24
    cc.check_case_set(c)
    assert len(c["V"]) <= 35                # (a batch of the GPU tests)
