"""GPU: the revised form of the LP engine keeps an age per slot (rank-1 steps on its basis inverse since it was built from the identity)
and, with bslv_lpq_set_refactor_period(K), refactorises an LP inside a solve once its inverse is K steps old -- at the start of a call
for children of an old parent, at the status readbacks for running LPs, which then go on.

Models, helpers and tolerances are those of tests/test_lp_refactor_gpu.py: "main" 40 x 300 (M 47, N 304, B 24) and "wide" 120 x 6000
with six dense columns (B 8); _close (objective 1e-9 relative, w and y 1e-7) and _bound (residual of a rebuilt inverse)."""
import os
import subprocess

import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.lp import P2Model, LpEngine
from test_lp_refactor_gpu import (OPTIMAL, ROOT, _P1Model, _bound, _close, _env, _first_generation, _problem, _read, _read_img, _reference,
                                  _residual, _rho_ref, _same_bits, _second_generation, _sparse_covering)

pytestmark = pytest.mark.gpu
KP = 6                # pivots between two passes (KP of lp_engine.hip): the bound on the age is 2 K + KP
ZERO = dict(at_start=0, in_rounds=0, replay_pivots=0, max_age=0)
CLEAN = dict(BSLV_LP_REFACTOR=None, BSLV_LP_REV_DRIFT=None, BSLV_LP_REFACTOR_EVERY=None)


def _engine(case, rev="1", **env):
    p = _problem(case)
    with _env(**dict(CLEAN, BSLV_LP_REV=rev, **env)):
        eng = LpEngine.from_model(p["model"], pool_slots=2 * p["B"] + 4)
    assert eng.rows_folded() == 0 and eng.lib.bslv_lpq_is_revised(eng.h) == int(rev)
    return eng


def _cold(eng, case):
    p = _problem(case)
    eng.reset_slot(0)
    st, it = eng.solve_batch([0], [0], np.full((1, p["model"].r), -np.inf), p["ub"][:1])
    assert st[0] == OPTIMAL, st
    return it


def _first(eng, case):
    p = _problem(case)
    B = p["B"]
    return eng.solve_batch(np.zeros(B, np.int32), p["dst"], np.full((B, p["model"].r), -np.inf), p["ub"])


def _second(eng, case):
    p = _problem(case)
    B = p["B"]
    return eng.solve_batch(p["dst"], p["dst2"], np.full((B, p["model"].r), -np.inf), p["ub2"])


# ---- 1. the switch ----
def test_switch_and_refusals():
    eng = _engine("main", rev="0")
    assert eng.set_refactor_period(5) == 2 and b"tableau" in eng.lib.bslv_last_error()          # BSLV_E_ARG
    assert eng.get_refactor_period() == 0
    assert eng.set_refactor_period(0) == 0
    assert eng.set_refactor_period(-1) == 2
    _cold(eng, "main")
    assert eng.slot_age(0) == 0                       # the tableau form reports 0
    eng.close()
    eng = _engine("main")
    assert eng.get_refactor_period() == 0             # off unless asked for
    assert eng.set_refactor_period(-1) == 2 and eng.get_refactor_period() == 0
    assert eng.set_refactor_period(5) == 0 and eng.get_refactor_period() == 5
    assert eng.set_refactor_period(0) == 0 and eng.get_refactor_period() == 0
    assert eng.set_refactor(1) == 0 and eng.set_refactor_period(3) == 0 and eng.get_refactor() == 1      # independent switches
    eng.close()
    eng = _engine("main", BSLV_LP_REFACTOR_EVERY="7")
    assert eng.get_refactor_period() == 7 and eng.get_refactor() == 0
    eng.close()
    eng = _engine("main", rev="0", BSLV_LP_REFACTOR_EVERY="7")      # (the tableau form ignores the variable)
    assert eng.get_refactor_period() == 0
    eng.close()


# ---- 2. the age ----
def test_age_of_a_slot():
    case = "main"
    p = _problem(case)
    model = p["model"]
    eng = _engine(case)
    eng.reset_slot(0)
    assert eng.slot_age(0) == 0
    _cold(eng, case)
    a0 = eng.slot_age(0)
    assert a0 == eng.last_stats()["pivots"] and a0 > 0
    free = np.full((1, model.r), -np.inf)
    st, it = eng.solve_batch([0], [1], free, p["ub"][1:2])                  # a child
    assert st[0] == OPTIMAL and it[0] > 0
    assert eng.slot_age(1) == a0 + int(it[0]) and eng.slot_age(0) == a0
    st, it2 = eng.solve_batch([1], [1], free, p["ub"][2:3])                 # in place adds
    assert st[0] == OPTIMAL and it2[0] > 0
    assert eng.slot_age(1) == a0 + int(it[0]) + int(it2[0])
    st, it3 = eng.solve_batch([0], [2], free, p["ub"][:1])                  # a child that makes no pivot inherits the age
    assert st[0] == OPTIMAL and it3[0] == 0 and eng.slot_age(2) == a0
    assert list(eng.refactor([1])) == [0]
    assert eng.slot_age(1) == 0 and eng.slot_age(0) == a0
    eng.debug_swap_heads(2, 3, 1)                                           # the heads change, the matrix does not
    assert eng.slot_age(2) == a0
    eng.refactor([2])                                                       # (whatever the new basis is: the slot is rebuilt or reset)
    assert eng.slot_age(2) == 0
    eng.reset_slot(0)
    assert eng.slot_age(0) == 0
    with pytest.raises(Exception, match="bad slot"):
        eng.slot_age(eng.pool_slots)
    eng.close()


# ---- 3. off changes nothing ----
def test_period_zero_changes_nothing():
    case = "main"
    p = _problem(case)
    ref = _reference(case)
    eng = _engine(case)
    assert eng.set_refactor_period(0) == 0
    _cold(eng, case)
    assert eng.last_period_stats() == ZERO
    st, it = _first(eng, case)
    assert np.all(st == OPTIMAL) and np.array_equal(it, ref["it"])
    assert eng.last_period_stats() == ZERO
    first = _read(eng, p["model"], p["dst"])
    st2, it2 = _second(eng, case)
    assert np.all(st2 == OPTIMAL) and np.array_equal(it2, ref["it2"])
    assert eng.last_period_stats() == ZERO
    second = _read(eng, p["model"], p["dst2"])
    for k in ("obj", "w", "y"):
        assert _same_bits(first[k], ref["first"][k]) and _same_bits(second[k], ref["second"][k]), k
    eng.close()


# ---- 4. equivalence while solving ----
def _check_slots(eng, case, slots):
    p = _problem(case)
    for s in slots:
        h, X = eng.get_inverse(int(s))
        rho_ref, res = _rho_ref(p, h), _residual(p, h, X)
        print("lp_period_residual case %s slot %d age %d rho_ref %.3e residual %.3e" % (case, s, eng.slot_age(int(s)), rho_ref, res))
        assert res <= _bound(rho_ref), (case, s, res, rho_ref)


def _generations(case, K, check=True):
    """cold solve, first and second generation with the period K; what a determinism check compares"""
    p = _problem(case)
    model = p["model"]
    eng = _engine(case)
    assert eng.set_refactor_period(K) == 0
    out = dict(stats=[], it=[], res=[])
    for name, run, slots in (("cold", _cold, [0]), ("first", _first, p["dst"]), ("second", _second, p["dst2"])):
        r = run(eng, case)
        st, it = (np.array([OPTIMAL]), r) if name == "cold" else r
        stats, ls = eng.last_period_stats(), eng.last_stats()
        print("lp_period case %s K %d %s: pivots %d rounds %d passes %d period %s" % (case, K, name, ls["pivots"], ls["lockstep_iters"], ls["passes"], stats))
        assert np.all(st == OPTIMAL), (name, st)
        assert ls["pivots"] == int(it.sum())
        assert stats["max_age"] <= 2 * K + KP, (name, stats)
        if name == "cold":
            assert stats["in_rounds"] >= 1, stats             # (both shapes make more than 20 pivots from the standard basis)
        if check:
            _check_slots(eng, case, slots)
            for s in slots:
                assert 0 <= eng.slot_age(int(s)) <= 2 * K + KP
        out["stats"].append(stats); out["it"].append(it.copy()); out["res"].append(_read(eng, model, slots))
    eng.close()
    return out


@pytest.mark.parametrize("K", [6, 20])
@pytest.mark.parametrize("case", ["main", "wide"])
def test_solves_with_a_period_equal_the_reference(case, K):
    """pivot counts may differ from the reference run -- the rounding differs -- so they are not compared"""
    ref = _reference(case)
    out = _generations(case, K)
    _close(out["res"][1], ref["first"])
    _close(out["res"][2], ref["second"])


# ---- 5. only some are due, and they are no prefix of the batch ----
def test_due_lps_between_lps_that_are_not():
    case = "main"
    p = _problem(case)
    model, B = p["model"], p["B"]
    eng = _engine(case)
    _cold(eng, case)
    a0 = eng.slot_age(0)
    assert a0 >= 2
    free = np.full((B, model.r), -np.inf)
    st, it = eng.solve_batch([0], [1], free[:1], p["ub"][:1])               # the same basis in slot 1 ...
    assert st[0] == OPTIMAL and it[0] == 0
    assert list(eng.refactor([1])) == [0]                                   # ... on a matrix of age 0
    assert eng.slot_age(1) == 0 and eng.slot_age(0) == a0
    assert np.array_equal(np.sort(eng.get_inverse(0, matrix=False)[0]), np.sort(eng.get_inverse(1, matrix=False)[0]))
    src = np.where(np.arange(B) % 2 == 1, 0, 1).astype(np.int32)            # odd LPs from the aged slot, even ones from the fresh one
    dst = np.arange(2, B + 2, dtype=np.int32)
    st, it = eng.solve_batch(src, dst, free, p["ub"])
    assert np.all(st == OPTIMAL) and eng.last_period_stats() == ZERO
    off = _read(eng, model, dst)
    assert eng.set_refactor_period(a0) == 0                                 # between the two ages: 0 < K <= a0
    st, it = eng.solve_batch(src, dst, free, p["ub"])
    stats = eng.last_period_stats()
    print("lp_period partial batch: K %d period %s" % (a0, stats))
    assert np.all(st == OPTIMAL), st
    assert stats["at_start"] == B // 2, stats
    _close(_read(eng, model, dst), off)
    ages = np.array([eng.slot_age(int(s)) for s in dst])
    assert np.array_equal(ages[1::2], it[1::2]) or stats["in_rounds"] > 0   # a refactorised child carries its own pivots only
    _check_slots(eng, case, dst)
    eng.close()


# ---- 6. repair at the start of a call ----
@pytest.mark.parametrize("case", ["main", "wide"])
def test_children_of_perturbed_parents_are_rebuilt_at_the_start(case):
    """every first-generation slot gets a drifted inverse (debug_perturb_inverse); with K = 1 every child is refactorised in its own
    slot before its first selection, and no child reads the perturbed numbers: the second generation is the reference's"""
    p = _problem(case)
    ref = _reference(case)
    eng, st, _ = _first_generation(case)
    assert np.all(st == OPTIMAL), st
    for s in p["dst"]:
        eng.debug_perturb_inverse(s, 1e-6)
        h, X = eng.get_inverse(s)
        assert _residual(p, h, X) >= 1e-7, "the perturbation hook did not change the stored inverse"
        assert eng.slot_age(int(s)) >= 1
    assert eng.set_refactor_period(1) == 0
    second, _ = _second_generation(eng, case)                               # (asserts that all are OPTIMAL)
    stats = eng.last_period_stats()
    print("lp_period start repair case %s: %s" % (case, stats))
    assert stats["at_start"] == p["B"], stats
    _close(second, ref["second"])
    _check_slots(eng, case, p["dst2"])
    eng.close()


def test_a_singular_basis_ends_undefined_beside_a_healthy_lp():
    """the failure path: heads that name a singular basis (debug_swap_heads on a copy of the solved slot, an exchange numpy finds
    singular) under a matrix old enough to be due.  The replay gives that LP up -- UNDEFINED, its dst slot reset -- while the LP next
    to it in the batch, due as well, is refactorised and solved.  An exchange that k_prep itself refuses never reaches the replay (the
    dst slot then keeps the copied heads): the next candidate is taken."""
    case = "main"
    p = _problem(case)
    model, M, N = p["model"], p["model"].M, p["model"].N
    eng = _engine(case)
    _cold(eng, case)
    free = np.full((2, model.r), -np.inf)
    ub = np.vstack([p["ub"][1], p["ub"][0]])
    st, _ = eng.solve_batch([0], [5], free[:1], p["ub"][:1])
    assert st[0] == OPTIMAL and eng.slot_age(5) == eng.slot_age(0) >= 1
    st, _ = eng.solve_batch([0, 0], [6, 7], free, ub)
    assert np.all(st == OPTIMAL)
    off = _read(eng, model, [6])
    assert eng.set_refactor_period(1) == 0
    reached = False
    for r, q in [(r, q) for r in range(0, M, 3) for q in range(0, N, 29)][:60]:
        eng.debug_swap_heads(5, r, q)
        h = eng.get_inverse(5, matrix=False)[0]
        if np.linalg.matrix_rank(p["K"][:, h]) == M:
            eng.debug_swap_heads(5, r, q)                       # (the same exchange undoes it)
            continue
        st, _ = eng.solve_batch([0, 5], [6, 7], free, ub)
        stats = eng.last_period_stats()
        assert st[0] == OPTIMAL and st[1] == 3, st               # UNDEFINED
        _close(_read(eng, model, [6]), off)
        h7, X7 = eng.get_inverse(7)
        if np.array_equal(h7, np.arange(M)):                    # the replay ran and failed: the slot is as after reset_slot
            assert _same_bits(X7, np.eye(M)) and eng.slot_age(7) == 0
            assert stats["at_start"] == 1, stats                # (the healthy LP; a failed replay is not counted)
            reached = True
            break
        assert np.array_equal(h7, h)                            # refused by k_prep
        eng.debug_swap_heads(5, r, q)
    assert reached, "no singular exchange reached the replay"
    st, _ = eng.solve_batch([0], [7], free[:1], p["ub"][:1])    # the engine goes on as before
    assert st[0] == OPTIMAL
    eng.close()


# ---- 7. across a cost perturbation ----
def _degenerate_sparse(m, n, q, seed, per_col=3):
    """the hypercube model of synth.degenerate_vlp with a sparse integer G: ties in every ratio test"""
    prob = synth.degenerate_vlp(m, n, q, seed)
    rng = np.random.default_rng(seed)
    g = m - n
    G = np.zeros((g, n))
    for j in range(n):
        rows = rng.choice(g, size=per_col, replace=False)
        G[rows, j] = rng.integers(1, 3, size=per_col)
    for i in range(g):
        while np.count_nonzero(G[i]) < 2:
            G[i, rng.integers(n)] = 1.0
    A = np.vstack([np.eye(n), G])
    return dict(prob, A=A)


def test_refactorisation_while_the_costs_are_perturbed(oracle):
    """extended selection, BSLV_STALL_LIMIT=1, integer data: in ONE call a cost perturbation starts and running LPs are refactorised;
    the results are those of the same call without a period and of the oracle LP solved from scratch"""
    import oracle_api
    m, n, q, seed, B, K = 100, 40, 3, 3, 12, 6
    prob = _degenerate_sparse(m, n, q, seed)
    model = P2Model(prob)
    rng = np.random.default_rng(seed)
    V = (rng.uniform(0.2, 0.9, size=(B, n)) @ prob["P"].T) + rng.normal(scale=0.3, size=(B, q))
    ub = model.ub_for(V)
    free = np.full((B, model.r), -np.inf)
    runs = {}
    for period in (0, K):
        with _env(**dict(CLEAN, BSLV_LP_REV="1", BSLV_STALL_LIMIT="1")):
            eng = LpEngine.from_model(model, pool_slots=B + 1)
            assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
            eng.set_extended(1)
            assert eng.set_refactor_period(period) == 0
            eng.reset_slot(0)
            dst = np.arange(1, B + 1, dtype=np.int32)
            st, it = eng.solve_batch(np.zeros(B, np.int32), dst, free, ub)     # B cold solves in one call
        ls, stats = eng.last_stats(), eng.last_period_stats()
        print("lp_period perturbed: period %d pivots %d perturbations %d primal steps %d period %s" % (period, ls["pivots"], ls["perturbations"], ls["primal_steps"], stats))
        assert np.all(st == OPTIMAL), st
        if period:
            assert ls["perturbations"] > 0 and stats["in_rounds"] > 0, (ls, stats)
            assert stats["max_age"] <= 2 * K + KP
        runs[period] = _read(eng, model, dst)
        eng.close()
    _close(runs[K], runs[0])
    olp = oracle_api.OracleLP(model.L, model.lo, model.up, model.cost)
    exp = np.empty(B)
    for b in range(B):
        for j in range(model.r):
            olp.set_bound(model.var_first + j, -np.inf, ub[b, j])
        assert olp.solve(1) == OPTIMAL
        exp[b] = olp.obj()
    olp.close()
    np.testing.assert_allclose(runs[K]["obj"], exp, rtol=1e-9, atol=1e-9)


# ---- 8. objective batches ----
def _obj_run(model, prob, W, W2, K):
    """the chain of _obj_chain -- feasibility LP, in place, batch from slot 0 -- and a second generation, with the period K"""
    from test_lp_rev_obj_gpu import _check_certificates
    B = len(W)
    with _env(**dict(CLEAN, BSLV_LP_REV="1")):
        eng = LpEngine(model.M, model.N, model.L, model.lo, model.up, np.zeros(model.N + 1), 0, 0, 2 * B + 2)
    assert eng.lib.bslv_lpq_is_revised(eng.h) == 1
    assert eng.set_refactor_period(K) == 0
    made = 0
    eng.reset_slot(0)
    st, _ = eng.solve_batch([0], [0], np.zeros((1, 0)), np.zeros((1, 0)))
    assert st[0] == OPTIMAL
    st, _ = eng.solve_batch_obj([0], [0], model.y_first, np.full((1, model.q), 1.0 / model.q))
    assert st[0] == OPTIMAL
    s = eng.last_period_stats(); made += s["at_start"] + s["in_rounds"]
    dst, dst2 = np.arange(1, B + 1, dtype=np.int32), np.arange(B + 1, 2 * B + 1, dtype=np.int32)
    out = {}
    for name, src, d, w in (("first", np.zeros(B, np.int32), dst, W), ("second", dst, dst2, W2)):
        st, it = eng.solve_batch_obj(src, d, model.y_first, w)
        s = eng.last_period_stats(); made += s["at_start"] + s["in_rounds"]
        print("lp_period objective batch K %d %s: pivots %d period %s" % (K, name, int(it.sum()), s))
        assert np.all(st == OPTIMAL), st
        assert s["max_age"] <= 2 * K + KP or K == 0
        obj = eng.obj(d).copy()
        _check_certificates(model, prob, eng, d, w, obj)                    # strong duality at 1e-8 among them
        out[name] = dict(obj=obj, y=eng.primal(d, model.y_first, model.q).copy(), w=eng.dual(d, 0, model.m).copy())
    eng.close()
    return out, made


def test_objective_batches_with_a_period():
    m, n, q, seed, B = 40, 300, 3, 5, 16
    rng = np.random.default_rng(seed)
    base = synth.covering_vlp(m, n, q, seed)
    prob = _sparse_covering(m, n, q, seed)
    mask = prob["P"] != 0
    mask[rng.integers(q, size=n), np.arange(n)] = True      # (a column of P without a non-zero would make y = 0 optimal for every w >= 0)
    prob = dict(prob, P=base["P"] * mask)
    model = _P1Model(prob)
    W = rng.uniform(0.1, 1.0, size=(B, q))
    W /= W.sum(axis=1, keepdims=True)
    W2 = np.abs(W * rng.uniform(0.8, 1.2, size=W.shape))
    W2 /= W2.sum(axis=1, keepdims=True)
    off, made0 = _obj_run(model, prob, W, W2, 0)
    on, made = _obj_run(model, prob, W, W2, 6)
    assert made0 == 0 and made > 0
    for name in ("first", "second"):
        _close(on[name], off[name])            # (w here: the duals of the cover rows)


# ---- 9. determinism ----
def test_runs_with_a_period_are_deterministic():
    a, b = _generations("main", 6, check=False), _generations("main", 6, check=False)
    assert a["stats"] == b["stats"]
    for k in range(3):
        assert np.array_equal(a["it"][k], b["it"][k])
        for f in ("obj", "w", "y"):
            assert _same_bits(a["res"][k][f], b["res"][k][f]), (k, f)


@pytest.mark.parametrize("case", ["main", "wide"])
def test_explicit_and_periodic_rebuild_are_the_same_replay(case):
    """the same basis -- a child of the cold solve with the cold solve's own bounds, which makes no pivot -- rebuilt by bslv_lpq_refactor
    and by the periodic refactorisation at the start of the call that makes the child: the same heads, and the same bits in the inverse
    and in what the getters read from the slot"""
    p = _problem(case)
    model = p["model"]
    free = np.full((1, model.r), -np.inf)
    got = {}
    for how in ("explicit", "periodic"):
        eng = _engine(case)
        _cold(eng, case)
        if how == "periodic":
            assert eng.set_refactor_period(1) == 0
        st, it = eng.solve_batch([0], [2], free, p["ub"][:1])
        assert st[0] == OPTIMAL and it[0] == 0, (how, st, it)
        if how == "explicit":
            assert list(eng.refactor([2])) == [0]
        else:
            assert eng.last_period_stats()["at_start"] == 1, eng.last_period_stats()
        assert eng.slot_age(2) == 0, how
        got[how] = (eng.get_inverse(2), _read(eng, model, [2]))
        eng.close()
    (ha, Xa), ra = got["explicit"]
    (hb, Xb), rb = got["periodic"]
    assert np.array_equal(ha, hb)
    assert _same_bits(Xa, Xb)
    for k in ("obj", "w", "y"):
        assert _same_bits(ra[k], rb[k]), k


# ---- 10. with the rescue on as well ----
def test_period_and_rescue_together():
    """the parent is aged (cold solve without a period), so with K = 6 every child is refactorised at the start; the cross-check of one
    LP is taken as failed at its first pivot and the rescue refactorises and solves it again: two counters, kept apart"""
    case = "main"
    p = _problem(case)
    ref = _reference(case)
    b = int(np.nonzero(ref["it"] >= 4)[0][0])
    eng = _engine(case)
    _cold(eng, case)
    assert eng.slot_age(0) >= 6
    assert eng.set_refactor(1) == 0 and eng.set_refactor_period(6) == 0
    with _env(BSLV_LP_REV_DRIFT="%d:1" % b):
        st, it = _first(eng, case)
    assert np.all(st == OPTIMAL), st
    rf, per = eng.last_refactor_stats(), eng.last_period_stats()
    print("lp_period with rescue: refactor %s period %s" % (rf, per))
    assert rf["rescued"] == 1 and rf["refactorised"] == 1 and rf["failed"] == 0, rf
    assert per["at_start"] == p["B"] and per["replay_pivots"] > rf["replay_pivots"], (per, rf)
    assert eng.last_stats()["pivots"] == int(it.sum())
    _close(_read(eng, p["model"], p["dst"]), ref["first"])
    eng.close()


# ---- 11. the drivers ----
PERIOD_ENV = dict(BSLV_LP_REV="1", BSLV_LP_REFACTOR_EVERY="6")


@pytest.mark.parametrize("alg", ["primal", "dual"])
def test_benson_run_with_a_period(alg):
    import poly_harness as ph
    from bensolve_amd.vlp import solve_primal
    prob = synth.covering_vlp(30, 15, 3, 5)
    with _env(**dict(CLEAN, BSLV_LP_REV=None)):
        a = solve_primal(prob, bounded=True, batch=32, eps_benson_phase2=1e-9, alg_phase2=alg)
    with _env(**dict(CLEAN, **PERIOD_ENV)):
        b = solve_primal(prob, bounded=True, batch=32, eps_benson_phase2=1e-9, alg_phase2=alg)
    assert a["status"] == b["status"] == "optimal", (a["message"], b["message"])
    ph.assert_benson_results_agree(ph.canonical(b["dump"], decimals=6), ph.canonical(a["dump"], decimals=6))


@pytest.mark.parametrize("alg", ["primal", "dual"])
@pytest.mark.parametrize("ex", ["ex01", "ex05"])
def test_cli_with_a_period_matches_hybrid_goldens(tmp_path, ex, alg):
    cli = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "hybrid.npz"))
    base = os.path.join(tmp_path, ex)
    env = {k: v for k, v in os.environ.items() if k not in CLEAN}
    r = subprocess.run([cli, os.path.join(ROOT, "tests", "golden", "ex", ex + ".vlp"), "-m", "2", "-B", "64", "-a", alg, "-o", base],
                       capture_output=True, text=True, timeout=600, env=dict(env, **PERIOD_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    for side in ("p", "d"):
        a = np.array([[float(x) for x in l.split()] for l in open(base + "_img_%s.sol" % side).read().strip().splitlines()])
        t, X = _read_img(a[:, 0].astype(int), a[:, 1:])
        gt, gX = _read_img(gold["%s/%s_type" % (ex, side)], gold["%s/%s" % (ex, side)])
        assert np.array_equal(t, gt), (ex, side, r.stdout)
        np.testing.assert_allclose(X, gX, rtol=1e-9, atol=1e-9)
