"""GPU: objective batches under a simplex method of their own (bslv_lpq_solve_batch_obj_method: PRIMAL, DUAL, REPAIR) in both forms of
the LP engine -- the tableau form in this process (BSLV_LP_REV unset), the revised form in ONE fresh child process with BSLV_LP_REV=1
that runs every revised case and hands its records back (`python tests/test_lp_obj_method_gpu.py child FILE`).

Cases: lp_cases.objective_set(M, N, rng_name), generation 1, 16 LPs in one batch from the feasibility basis in slot 0, at the shapes
tests/test_lp_obj_general_gpu.py walks (its SHAPES for the tableau form, its REV_SHAPES for the revised form: the row lengths on both
sides of the wave, workgroup, slice and extended-selection thresholds listed there; every one of them is the smallest on its side).
Range "cols" everywhere -- the only one the two largest shapes run (lp_cases.obj_ranges), a cost on every nonbasic column -- and
"straddle" (costs on row variables too) at the two SIDE_SHAPES.

References: lp_cases.objective_references (the CPU oracle's primal simplex and HiGHS), never the engine's own PRIMAL result; the bounds
on the residuals are lp_cases.assert_certified / gap_bound's, and every OPTIMAL slot also has to pass the engine's own certificate
(bslv_lpq_certify, default tolerances: the same figures).

NOT VACUOUS: before the GPU is touched the oracle says, per set, how many LPs have a parent basis (the oracle's feasibility basis) that
is dual infeasible for the new cost, and whether each of those has a column to move (a boxed nonbasic column on the wrong side): at
least half of the LPs, each with at least one.  On the GPU every set must then report moved columns and an LP with a dual pivot.

THE POLISH.  Most LPs of these sets start on artificial bounds of the call (free and one-sided columns whose new reduced cost points
where they have no bound), and an LP that does and ends OPTIMAL is solved once more inside the call as a PRIMAL objective batch in its
own slot (include/bslv_hip.h).  What these tests certify of such an LP is therefore the point and the basis the call RETURNS -- after
the polish -- while the counters (LPs started dual, variables moved, dual pivots) are the dual start's.  Without the polish the
returned points lay 1e7 away on the optimal face (190 - 375 of 1024 variables per LP at (24, 1024)) and the row residuals were
1.6e-8 ... 2.4e-5; with it all cases of this file pass on the MI355X, row residuals 1e-13 ... 3e-12."""
import ctypes
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lp_cases as lc
from lp_cases import RTOL, OPTIMAL, UNBOUNDED, UNDEFINED, NLP
from test_lp_general_gpu import _engine, _read, _assert_identical
from test_lp_obj_general_gpu import SHAPES, REV_SHAPES, SIDE_SHAPES, _feasible_start, _assert_against_references

pytestmark = pytest.mark.gpu

DUAL, PRIMAL, REPAIR = 0, 1, 2
NONE = np.zeros((1, 0))
FREE_SHAPE = (32, 65)           # the free-column model: general_set's arrangement "b" (columns 1 .. 40 per LP, free ones among them)


def _sets(shapes):
    return [(M, N, r) for M, N in shapes for r in (("cols", "straddle") if (M, N) in SIDE_SHAPES else ("cols",))]


TAB_SETS, REV_SETS = _sets(SHAPES), _sets(REV_SHAPES)
# slots: 0 the parent; then one block of 16 per solve
BASE, PRIM, DUA, REP, INPL, DVX_D, DVX_R = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(7))
POOL = 1 + 7 * NLP
STAT_KEYS = ("phase1_lps", "phase1_iterations", "phase1_rebuilds", "init_chunks", "lockstep_iters", "pivots", "passes", "launches", "flip_iterations",
             "perturbations", "primal_steps", "wrong_sign_removals", "flip_vector_updates")


# ---- the CPU side ---------------------------------------------------------------------------------------------------------------
class _OLP(ctypes.Structure):
    """the head of oracle/lp_dense.c's struct olp, read-only: the basis the oracle stands on after a solve"""
    _fields_ = [("M", ctypes.c_int), ("N", ctypes.c_int), ("A", ctypes.c_void_p), ("rtype", ctypes.c_void_p), ("ctype", ctypes.c_void_p),
                ("rlb", ctypes.c_void_p), ("rub", ctypes.c_void_p), ("clb", ctypes.c_void_p), ("cub", ctypes.c_void_p), ("c", ctypes.c_void_p),
                ("valid", ctypes.c_int), ("T", ctypes.POINTER(ctypes.c_double)), ("bh", ctypes.POINTER(ctypes.c_int)), ("nh", ctypes.POINTER(ctypes.c_int)),
                ("nstat", ctypes.POINTER(ctypes.c_int))]


_COUNTS = {}


def _oracle_counts(M, N, rng_name):
    """with the oracle, no GPU: (LPs of generation 1 whose parent basis -- the oracle's basis of the feasibility LP -- is dual infeasible
    for the new cost, those of them with at least one boxed nonbasic column on the wrong side)"""
    key = (M, N, rng_name)
    if key in _COUNTS:
        return _COUNTS[key]
    import oracle_api
    s = lc.objective_set(M, N, rng_name)
    o = oracle_api.OracleLP(s["A"], s["lo"], s["up"], np.zeros(N + 1))
    assert o.solve(1) == OPTIMAL
    h = ctypes.cast(o.h, ctypes.POINTER(_OLP)).contents
    assert (h.M, h.N) == (M, N)
    T = np.ctypeslib.as_array(h.T, (M, N)).copy()
    bh, nh, ns = (np.ctypeslib.as_array(p, (n,)).copy() for p, n in ((h.bh, M), (h.nh, N), (h.nstat, N)))
    o.close()
    lo, up = s["lo"][nh], s["up"][nh]
    boxed = np.isfinite(lo) & np.isfinite(up) & (lo < up)
    infeasible = movable = 0
    for c in s["costs"]["gen1"]:
        full = np.zeros(M + N)
        full[s["cost_first"]:s["cost_first"] + s["cost_cnt"]] = c
        d = full[nh] + full[bh] @ T            # (lp_dense.c refresh_d)
        wrong = ((ns == 0) & (d < -1e-9)) | ((ns == 1) & (d > 1e-9)) | ((ns == 2) & (np.abs(d) > 1e-9))      # (its dual_feasible)
        infeasible += bool(wrong.any())
        movable += bool((wrong & boxed).any())
    _COUNTS[key] = (infeasible, movable)
    return _COUNTS[key]


def _assert_not_vacuous_on_the_cpu(M, N, rng_name):
    infeasible, movable = _oracle_counts(M, N, rng_name)
    assert 2 * infeasible >= NLP and movable == infeasible, (M, N, rng_name, infeasible, movable)


def _reduced_costs(A, vstat, row_of, full_cost):
    """d over all variables (0 on the basic ones) for the basis of bslv_lpq_get_basis, K = [I | -A]: d_j = c_j - y . K_j, y B = c_B"""
    M, N = A.shape
    K = np.hstack([np.eye(M), -A])
    basic = np.nonzero(vstat == 1)[0]
    Bm = np.zeros((M, M))
    Bm[:, row_of[basic]] = K[:, basic]
    cB = np.zeros(M)
    cB[row_of[basic]] = full_cost[basic]
    y = np.linalg.solve(Bm.T, cB)
    d = full_cost - y @ K
    d[basic] = 0.0
    return d


def _unstartable(A, lo, up, vstat, row_of, full_cost, first, cnt):
    """is there a nonbasic variable of the per-LP range first .. first + cnt - 1 that no side makes dual feasible (include/bslv_hip.h,
    bslv_lpq_solve_batch_obj_method); None where a reduced cost lies between the two thresholds of the rule"""
    d = _reduced_costs(A, vstat, row_of, full_cost)
    k = np.arange(first, first + cnt)
    k = k[(vstat[k] != 1) & (lo[k] < up[k])]
    if np.any((np.abs(d[k]) > 1e-10) & (np.abs(d[k]) < 1e-6)):
        return None
    return bool(np.any(((d[k] > 1e-7) & np.isinf(lo[k])) | ((d[k] < -1e-7) & np.isinf(up[k]))))


# ---- the GPU side: one record per set and form -------------------------------------------------------------------------------------
def _solve(eng, method, dst, first, C, src=None, vlo=None, vup=None):
    st, it = eng.solve_batch_obj_method(method, np.zeros(len(dst), np.int32) if src is None else src, dst, first, C, vlo, vup)
    got = _read(eng, dst, st, it)
    got["stats"] = eng.last_obj_method_stats()
    got["last"] = {k: v for k, v in eng.last_stats().items() if k in STAT_KEYS}
    got["verdict"] = eng.certify(dst, vlo, vup, cost_first=first, costs=C)["verdict"]
    return got


def _do_record(M, N, rng_name, form):
    s = lc.objective_set(M, N, rng_name)
    first, C = s["cost_first"], s["costs"]["gen1"]
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL, form)
    assert eng.rows_folded() == 0
    _feasible_start(eng, 0, NONE, NONE)
    rec = {}
    st, it = eng.solve_batch_obj(np.zeros(NLP, np.int32), BASE, first, C)
    rec["base"] = _read(eng, BASE, st, it)
    rec["base"]["last"] = {k: v for k, v in eng.last_stats().items() if k in STAT_KEYS}
    rec["base"]["stats"] = eng.last_obj_method_stats()
    rec["primal"] = _solve(eng, PRIMAL, PRIM, first, C)
    rec["dual"] = _solve(eng, DUAL, DUA, first, C)
    rec["repair"] = _solve(eng, REPAIR, REP, first, C)
    for b in INPL:          # in place: every slot holds the feasibility solution, then is its own parent
        _feasible_start(eng, b, NONE, NONE)
    rec["inplace"] = _solve(eng, REPAIR, INPL, first, C, src=INPL)
    assert eng.set_pricing(1) == 0
    rec["devex_dual"] = _solve(eng, DUAL, DVX_D, first, C)
    rec["devex_repair"] = _solve(eng, REPAIR, DVX_R, first, C)
    rec["devex_used"] = eng.last_pricing_stats()
    eng.close()
    return rec


def _do_unbounded(M, N, form):
    s = lc.unbounded_objective_set(M, N)
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, POOL, form)
    assert eng.set_rays(1) == 0
    _feasible_start(eng, 0, NONE, NONE)
    rec = {}
    for name, method, dst in (("primal", PRIMAL, PRIM), ("dual", DUAL, DUA), ("repair", REPAIR, REP)):
        got = _solve(eng, method, dst, s["cost_first"], s["costs"])
        kind, _ = eng.get_ray(dst, vectors=False)
        cert = eng.certify_rays(dst, cost_first=s["cost_first"], costs=s["costs"])
        got["ray_kind"], got["ray_verdict"] = kind, cert["verdict"]
        rec[name] = got
    eng.close()
    return rec


def _do_free(form):
    """the free-column model: general_set(.., "b") -- columns 1 .. 40 get their bounds per LP, free and one-sided ones among them, and
    get no artificial bound -- under the costs of the objective set of the same shape; every LP has the bounds of LP 0, the model's"""
    M, N = FREE_SHAPE
    s, g = lc.objective_set(M, N, "cols"), lc.general_set(M, N, "b")
    vlo, vup = np.tile(g["vlo"][0], (NLP, 1)), np.tile(g["vup"][0], (NLP, 1))
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], g["var_first"], g["var_cnt"], POOL, form)
    _feasible_start(eng, 0, vlo[:1], vup[:1])
    vstat, row_of = eng.get_basis(0)
    rec = dict(vstat=vstat, row_of=row_of)
    for name, method, dst in (("dual", DUAL, DUA), ("repair", REPAIR, REP)):
        rec[name] = _solve(eng, method, dst, s["cost_first"], s["costs"]["gen1"], vlo=vlo, vup=vup)
    eng.close()
    return rec


_RECORDS = {}


def _child_records():
    """every revised-form record, from one fresh process that has BSLV_LP_REV=1 in its environment"""
    if "child" not in _RECORDS:
        fd, path = tempfile.mkstemp(suffix=".pkl")
        os.close(fd)
        try:
            env = dict(os.environ, BSLV_LP_REV="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=env, capture_output=True, text=True, timeout=600)
            assert "Memory access fault" not in p.stderr, p.stderr[-800:]
            assert p.returncode == 0, "rc %d\n%s" % (p.returncode, p.stderr[-2000:])
            with open(path, "rb") as f:
                _RECORDS["child"] = pickle.load(f)
        finally:
            os.unlink(path)
    return _RECORDS["child"]


def _child(path):
    assert os.environ.get("BSLV_LP_REV") == "1"
    out = {("set",) + k: _do_record(*k, "revised") for k in REV_SETS}
    for M, N in SIDE_SHAPES:
        out[("unbounded", M, N)] = _do_unbounded(M, N, "revised")
    out[("free",)] = _do_free("revised")
    with open(path, "wb") as f:
        pickle.dump(out, f)


def _record(kind, form, *key):
    if form == "revised":
        return _child_records()[(kind,) + key]
    k = (kind, form) + key
    if k not in _RECORDS:
        assert os.environ.get("BSLV_LP_REV") is None
        _RECORDS[k] = {"set": _do_record, "unbounded": _do_unbounded, "free": _do_free}[kind](*key, form)
    return _RECORDS[k]


def _cases():
    return [pytest.param(M, N, r, "tableau", id="tableau-%d-%d-%s" % (M, N, r)) for M, N, r in TAB_SETS] + \
           [pytest.param(M, N, r, "revised", id="revised-%d-%d-%s" % (M, N, r)) for M, N, r in REV_SETS]


# ---- 1. PRIMAL is solve_batch_obj -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rng_name,form", _cases())
def test_primal_is_solve_batch_obj_byte_for_byte(M, N, rng_name, form):
    rec = _record("set", form, M, N, rng_name)
    a, b = rec["base"], rec["primal"]
    for k in ("st", "it", "obj", "prim", "dual"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (form, M, N, rng_name, k)
    assert a["last"] == b["last"], (a["last"], b["last"])
    assert a["stats"] == b["stats"] == [0, 0, 0, 0]


# ---- 2. DUAL and REPAIR against the references -------------------------------------------------------------------------------------
def _check_method(M, N, rng_name, form, name):
    _assert_not_vacuous_on_the_cpu(M, N, rng_name)
    s = lc.objective_set(M, N, rng_name)
    ref, oracle, _ = lc.assert_objective_references_agree(M, N, rng_name)
    got = _record("set", form, M, N, rng_name)[name]
    tag = (form, M, N, rng_name, name)
    print("pivots %s: %s; started dual %d, variables moved %d, handed to the primal start %d, dual pivots %d" % ((tag, got["it"]) + tuple(got["stats"])))
    certs = _assert_against_references(s, s["folded"]["gen1"], ref["gen1"], oracle["gap"], got, tag)
    assert len(certs) == NLP
    assert np.all(got["verdict"][got["st"] == OPTIMAL] == 0), (tag, got["verdict"])      # (bslv_lpq_certify)
    return got


@pytest.mark.parametrize("M,N,rng_name,form", _cases())
def test_dual_matches_the_references(oracle, M, N, rng_name, form):
    got = _check_method(M, N, rng_name, form, "dual")
    assert got["stats"][0] == NLP and got["stats"][2] == 0, got["stats"]
    assert got["stats"][1] > 0 and np.any(got["it"] >= 1) and got["stats"][3] >= 1, got["stats"]
    assert got["last"]["primal_steps"] + got["stats"][3] == got["last"]["pivots"]


@pytest.mark.parametrize("M,N,rng_name,form", _cases())
def test_repair_matches_the_references(oracle, M, N, rng_name, form):
    got = _check_method(M, N, rng_name, form, "repair")
    assert got["stats"][0] + got["stats"][2] == NLP, got["stats"]
    assert got["stats"][1] > 0 and got["stats"][3] >= 1, got["stats"]


# ---- 3. in place, and under dual Devex pricing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,rng_name,form", _cases())
def test_in_place_and_out_of_place_agree_bit_for_bit(M, N, rng_name, form):
    rec = _record("set", form, M, N, rng_name)
    _assert_identical(rec["repair"], rec["inplace"], (form, M, N, rng_name, "in place"))
    assert np.array_equal(rec["repair"]["it"], rec["inplace"]["it"]) and rec["repair"]["stats"] == rec["inplace"]["stats"]


@pytest.mark.parametrize("M,N,rng_name,form", _cases())
def test_dual_devex_gives_the_same_statuses_and_values(M, N, rng_name, form):
    rec = _record("set", form, M, N, rng_name)
    for plain, dvx in (("dual", "devex_dual"), ("repair", "devex_repair")):
        assert np.array_equal(rec[plain]["st"], rec[dvx]["st"]), (form, M, N, rng_name, plain, rec[plain]["st"], rec[dvx]["st"])
        ok = rec[plain]["st"] == OPTIMAL
        np.testing.assert_allclose(rec[dvx]["obj"][ok], rec[plain]["obj"][ok], rtol=RTOL, atol=1e-9)
        assert np.all(rec[dvx]["verdict"][ok] == 0)
    assert rec["devex_used"]["weighted"] > 0, rec["devex_used"]          # (selections under the weighted rule: the Devex instance ran)


# ---- 4. unbounded objectives --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
@pytest.mark.parametrize("M,N", SIDE_SHAPES)
def test_unbounded_objectives_under_every_method(oracle, M, N, form):
    """a free column in no row: LPs 2, 5 and 9 put a cost on it.  DUAL and REPAIR report what PRIMAL reports, which is what both
    yardsticks say; a stored ray certifies or is absent (DUAL ends on an artificial bound of the call: UNBOUNDED without a ray, as
    solve_batch); REPAIR hands over exactly the LPs whose start cannot be made dual feasible -- none here, no variable has per-LP bounds"""
    s = lc.unbounded_objective_set(M, N)
    ref, oracle_w = lc.unbounded_objective_references(M, N)
    rec = _record("unbounded", form, M, N)
    want = [UNBOUNDED if t in lc.UNB_LPS else OPTIMAL for t in range(NLP)]
    for name in ("primal", "dual", "repair"):
        got = rec[name]
        tag = (form, M, N, "unbounded objectives", name)
        assert [int(v) for v in got["st"]] == want == [int(v) for v in rec["primal"]["st"]], (tag, got["st"])
        certs = _assert_against_references(s, s["folded"], ref, oracle_w["gap"], got, tag)
        assert len(certs) == NLP - len(lc.UNB_LPS)
        for t in range(NLP):
            assert got["ray_kind"][t] == 0 or (got["st"][t] == UNBOUNDED and got["ray_verdict"][t] == 0), (tag, t, got["ray_kind"], got["ray_verdict"])
    assert all(rec["primal"]["ray_kind"][t] == 2 and rec["primal"]["ray_verdict"][t] == 0 for t in lc.UNB_LPS)      # (the direction PRIMAL finds)
    assert rec["dual"]["stats"][0] == NLP and rec["repair"]["stats"][0] == NLP and rec["repair"]["stats"][2] == 0, (rec["dual"]["stats"], rec["repair"]["stats"])


# ---- 5. a start that cannot be made dual feasible -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tableau", "revised"])
def test_free_column_dual_is_undefined_where_repair_is_optimal(oracle, form):
    M, N = FREE_SHAPE
    s, g = lc.objective_set(M, N, "cols"), lc.general_set(M, N, "b")
    ref, oracle_w, _ = lc.assert_objective_references_agree(M, N, "cols")
    rec = _record("free", form)
    # the CPU says which LPs cannot start: from the parent's basis as the engine holds it, the model and the costs alone
    cannot = []
    for c in s["costs"]["gen1"]:
        full = np.zeros(M + N)
        full[s["cost_first"]:s["cost_first"] + s["cost_cnt"]] = c
        cannot.append(_unstartable(s["A"], s["lo"], s["up"], rec["vstat"], rec["row_of"], full, g["var_first"], g["var_cnt"]))
    assert None not in cannot, cannot
    assert any(cannot) and not all(cannot), cannot
    dual, repair = rec["dual"], rec["repair"]
    tag = (form, M, N, "free columns")
    assert [int(v) for v in dual["st"]] == [UNDEFINED if x else OPTIMAL for x in cannot], (tag, dual["st"], cannot)
    assert np.all(dual["it"][np.array(cannot)] == 0)
    assert np.all(repair["st"] == OPTIMAL), (tag, repair["st"])
    assert dual["stats"][0] == NLP - sum(cannot) and repair["stats"][0] == NLP - sum(cannot) and repair["stats"][2] == sum(cannot), (dual["stats"], repair["stats"], cannot)
    certs = _assert_against_references(s, s["folded"]["gen1"], ref["gen1"], oracle_w["gap"], repair, tag + ("repair",))
    assert len(certs) == NLP
    keep = [t for t in range(NLP) if not cannot[t]]
    _assert_against_references(s, s["folded"]["gen1"], ref["gen1"], oracle_w["gap"], {k: np.asarray(dual[k])[keep] for k in ("st", "it", "obj", "prim", "dual")}, tag + ("dual",), lps=keep)


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------------
def test_bad_method_is_refused_and_changes_nothing():
    M, N = 15, 16
    s = lc.objective_set(M, N, "cols")
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], 0, 0, 1 + NLP, "tableau")
    _feasible_start(eng, 0, NONE, NONE)
    st, it = eng.solve_batch_obj(np.zeros(NLP, np.int32), BASE, s["cost_first"], s["costs"]["gen1"])
    before = (_read(eng, BASE, st, it), eng.last_stats()["pivots"], eng.get_method())
    from bensolve_amd._lib import BslvError
    for bad in (-1, 3):
        with pytest.raises(BslvError):
            eng.solve_batch_obj_method(bad, np.zeros(NLP, np.int32), BASE, s["cost_first"], s["costs"]["gen1"])
    after = (_read(eng, BASE, st, it), eng.last_stats()["pivots"], eng.get_method())
    eng.close()
    _assert_identical(before[0], after[0], "refused call")
    assert before[1:] == after[1:]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        _child(sys.argv[2])
