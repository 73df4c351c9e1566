"""GPU: a basis put into a slot and taken out of one (include/bslv_hip.h: bslv_lpq_load_basis, bslv_lpq_get_basis, bslv_lpq_rebuild),
in the tableau form -- whose slot is rebuilt on the device by a replay of its own (bensolve_amd/csrc/lp_basis.inc) -- and in the revised
form, where the replay is bslv_lpq_refactor's.

Models: lp_cases.random_lp at the boundary shapes of tests/lp_cases.py, (24, 1536) for the 1024-thread workgroup of the replay's
selection, a 3 x 5 model and a 9 x 6 model of lp_cases whose presolve folds two rows (lp_basis_cases).  Bases: one per structural basic
count on the replay's edges -- 0, 1, KP - 1, KP, KP + 1, 2 KP + 1, M -- drawn seeded on the host and kept only where the host's float64
and longdouble solutions agree to 1e-11.  The solved bases come from lp_cases.general_set.

Every comparison with the host uses lp_cases.RTOL (1e-9) times 1 + max |.| of the vector compared; the certificate's thresholds are
the device certificate's defaults, which are lp_cases.certify's (TOL_ROWS ...).

Run as a program (`python tests/test_lp_basis_gpu.py child`) it loads the bases of two cases in both forms and prints a SHA-256 of
everything the getters return: the fill-byte test starts it that way under BSLV_FILL=0x7F."""
import contextlib
import ctypes
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bensolve_amd.lp import LpEngine
from bensolve_amd._lib import BslvError
import lp_cases as lc
import lp_basis_cases as bc
from lp_cases import RTOL, OPTIMAL, UNDEFINED, NLP

pytestmark = pytest.mark.gpu

SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 1121), (24, 1536)]
CASES = SHAPES + ["small", "folded"]
FORMS = ("tableau", "revised")
CHILD_CASES = ["small", (32, 65)]
NONE = np.zeros((1, 0))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(A, lo, up, cost, first, cnt, slots, form):
    M, N = A.shape
    with _env(BSLV_LP_REV="1" if form == "revised" else "0"):
        eng = LpEngine(M, N, A, lo, up, cost, first, cnt, slots)
    eng.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
    assert eng.lib.bslv_lpq_is_revised(eng.h) == int(form == "revised")
    return eng


def _read(eng, slots):
    n = eng.M + eng.N
    return dict(prim=eng.primal(slots, 0, n), dual=eng.dual(slots, 0, n), obj=eng.obj(slots))


def _bits(rec):
    return b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in ("prim", "dual", "obj"))


def _close(got, ref, tag):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, bound = float(np.max(np.abs(got - ref))), RTOL * (1.0 + float(np.max(np.abs(ref))))
    print("%s: max error %.3e, bound %.3e" % (tag, err, bound))
    assert err <= bound, (tag, err, bound)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the model as given, the engine's own model and the bases (own indices) of a case"""
    if name == "small":
        A, lo, up, cost = bc.small_model()
    elif name == "folded":
        A, lo, up, cost = bc.folded_model()
    else:
        A, lo, up, cost = bc.shape_model(*name)
    A2, lo2, up2, _, own = bc.own_model(A, lo, up, 0, 0)
    seed = 7 if isinstance(name, str) else 100 + name[0] + name[1]
    return dict(A=A, lo=lo, up=up, cost=cost, own=(A2, lo2, up2), own_of_given=own, bases=bc.bases(("gpu", name), A2, lo2, up2, cost, seed))


def _to_own(c, given_prim, given_dual):
    """the getters' vectors (model as given) in the engine's own indices.  A folded row's dual is the part of its column's reduced
    cost that belongs to the bound the row gave (get_mapped): the column's own-model reduced cost is the sum of the parts."""
    A, own = c["A"], c["own_of_given"]
    M, N = A.shape
    Mi = c["own"][0].shape[0]
    prim, dual = np.zeros(Mi + N), np.zeros(Mi + N)
    for v in range(M + N):
        if own[v] >= 0:
            prim[own[v]] = given_prim[v]
            dual[own[v]] += given_dual[v]
        else:
            j = int(np.nonzero(A[v])[0][0])
            dual[Mi + j] += given_dual[v] * A[v, j]
            np.testing.assert_allclose(given_prim[v], A[v, j] * given_prim[M + j], rtol=0, atol=1e-12)
    return prim, dual


@functools.lru_cache(maxsize=None)
def _loaded(name, form):
    """every basis of a case loaded once in one call, again in a second call, and into slots that hold an unrelated solved LP"""
    c = _case(name)
    nb = len(c["bases"])
    eng = _engine(c["A"], c["lo"], c["up"], c["cost"], 0, 0, 2 * nb + 1, form)
    try:
        first, dirty = np.arange(1, nb + 1, dtype=np.int32), np.arange(nb + 1, 2 * nb + 1, dtype=np.int32)
        vs = np.array([v for _, v, _ in c["bases"]], np.int32)
        rec = dict(nb=nb, folded=eng.rows_folded(), var_map=eng.var_map())
        for s in first:
            eng.reset_slot(int(s))
        rec["status"] = eng.load_basis(first, vs)
        rec["stats"] = eng.last_rebuild_stats()
        rec["one"] = _read(eng, first)
        rec["basis"] = [eng.get_basis(int(s)) for s in first]
        rec["status2"] = eng.load_basis(first, vs)
        rec["two"] = _read(eng, first)
        # slots that hold something else: the model's own LP, solved from the standard basis
        eng.reset_slot(0)
        st, it = eng.solve_batch(np.zeros(nb, np.int32), dirty, np.zeros((nb, 0)), np.zeros((nb, 0)))
        rec["dirty_solve"] = (st.copy(), it.copy())
        rec["status3"] = eng.load_basis(dirty, vs)
        rec["three"] = _read(eng, dirty)
        # the round trip: what get_basis returns, loaded into the slots again
        back = np.array([v for v, _ in rec["basis"]], np.int32)
        rec["status4"] = eng.load_basis(first, back)
        rec["four"] = _read(eng, first)
        rec["basis4"] = [eng.get_basis(int(s)) for s in first]
        return rec
    finally:
        eng.close()


# ---- 1. against the host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES, ids=str)
def test_loaded_bases_have_the_values_of_the_host(name, form):
    c, rec = _case(name), _loaded(name, form)
    assert np.all(rec["status"] == 0), rec["status"]
    assert rec["stats"] == dict(rebuilt=rec["nb"], replay_pivots=sum(ns for ns, _, _ in c["bases"]), passes=rec["stats"]["passes"], failed=0)
    assert rec["stats"]["passes"] >= rec["nb"]                 # (the refresh pass of every slot at least)
    assert np.array_equal(rec["var_map"], c["own_of_given"])
    assert rec["folded"] == (2 if name == "folded" else 0)
    for k, (ns, vstat, (z, d, obj)) in enumerate(c["bases"]):
        prim, dual = _to_own(c, rec["one"]["prim"][k], rec["one"]["dual"][k])
        tag = (name, form, ns)
        _close(prim, z, "%s primal" % (tag,))
        _close(dual, d, "%s dual" % (tag,))
        _close([rec["one"]["obj"][k]], [obj], "%s objective" % (tag,))
        # nonbasic values exactly
        non = vstat != bc.BASIC
        A2, lo2, up2 = c["own"]
        assert np.array_equal(prim[non], bc.nonbasic_values(vstat, lo2, up2)[non]), tag


# ---- 5. a function of the basis ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES, ids=str)
def test_the_result_is_a_function_of_the_basis(name, form):
    rec = _loaded(name, form)
    st, it = rec["dirty_solve"]
    if not isinstance(name, str):
        assert np.all(it > 0), (st, it)                          # (the slots really held something else)
    assert np.all(rec["status2"] == 0) and np.all(rec["status3"] == 0)
    assert _bits(rec["one"]) == _bits(rec["two"]), "a second call differs"
    assert _bits(rec["one"]) == _bits(rec["three"]), "a slot that held a solved LP differs from a reset one"


def _child_digest():
    h = hashlib.sha256()
    for name in CHILD_CASES:
        for form in FORMS:
            rec = _loaded(name, form)
            for k in ("one", "three", "four"):
                h.update(_bits(rec[k]))
            for v, r in rec["basis"]:
                h.update(v.tobytes())
    return h.hexdigest()


def test_loading_does_not_depend_on_the_fill_byte():
    """fresh device memory filled with 0x7F instead of zeros (the pattern of tests/test_fill_gpu.py): same bits"""
    env = dict(os.environ, BSLV_FILL="0x7F")
    env.pop("BSLV_LP_REV", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = [l for l in p.stdout.splitlines() if l.startswith("digest ")]
    assert got and got[-1] == "digest " + _child_digest(), (got, _child_digest())


# ---- 6. round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CASES, ids=str)
def test_get_basis_returns_what_was_loaded_and_loads_back(name, form):
    c, rec = _case(name), _loaded(name, form)
    Mi = c["own"][0].shape[0]
    assert np.all(rec["status4"] == 0)
    for k, (ns, vstat, _) in enumerate(c["bases"]):
        got, row_of = rec["basis"][k]
        assert np.array_equal(got, vstat), (name, form, ns)
        assert np.array_equal(row_of >= 0, vstat == bc.BASIC)
        assert sorted(row_of[row_of >= 0]) == list(range(Mi))
        got4, row_of4 = rec["basis4"][k]
        assert np.array_equal(got4, vstat)
        assert set(np.nonzero(row_of4 >= 0)[0]) == set(np.nonzero(row_of >= 0)[0])
    non = np.array([v for _, v, _ in c["bases"]]) != bc.BASIC
    if name != "folded":                                          # (own indices = given indices)
        assert np.array_equal(rec["four"]["prim"][non], rec["one"]["prim"][non])
    assert _bits(rec["four"]) == _bits(rec["one"])


# ---- 2, 3. solved bases: certificate, zero pivots, children -----------------------------------------------------------------
GEN1, LOADED, OUT_A, OUT_B = (np.arange(1 + k * NLP, 1 + (k + 1) * NLP, dtype=np.int32) for k in range(4))
POOL = 1 + 4 * NLP
SOLVED = [((15, 16), "a", "tableau"), ((16, 17), "a", "tableau"), ((31, 64), "a", "tableau"), ((32, 65), "a", "tableau"), ((32, 65), "b", "tableau"),
          ((33, 257), "a", "tableau"), ((24, 1121), "a", "tableau"), ((24, 1536), "a", "tableau"), ((24, 1536), "b", "tableau"),
          ((33, 257), "a", "revised"), ((24, 1536), "a", "revised")]


def _solve(eng, src, dst, vlo, vup, retry):
    """one batch; retry (the revised form): an LP that comes back UNDEFINED is solved once more from a reset slot, as the header tells
    callers to (tests/test_lp_general_gpu.py)"""
    st, it = eng.solve_batch(src, dst, vlo, vup)
    st, it = st.copy(), it.copy()
    if retry:
        for b in np.nonzero(st == UNDEFINED)[0]:
            eng.reset_slot(int(dst[b]))
            s1, i1 = eng.solve_batch([dst[b]], [dst[b]], vlo[b:b + 1], vup[b:b + 1])
            st[b], it[b] = s1[0], it[b] + i1[0]
    return st, it


def _gen1(eng, s, retry):
    eng.reset_slot(0)
    st, _ = _solve(eng, [0], [0], s["vlo"][:1], s["vup"][:1], retry)
    assert st[0] == OPTIMAL
    st, it = _solve(eng, np.zeros(NLP, np.int32), GEN1, s["vlo"], s["vup"], retry)
    return st, it


@functools.lru_cache(maxsize=None)
def _solved(shape, arr, form):
    s = lc.general_set(shape[0], shape[1], arr)
    vlo, vup, perm = s["vlo"], s["vup"], s["perm"]
    retry = form == "revised"
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, form)
    try:
        assert eng.rows_folded() == 0
        rec = {}
        st, it = _gen1(eng, s, retry)
        opt = np.nonzero(st == OPTIMAL)[0]
        rec.update(st=st, opt=opt, gen1=_read(eng, GEN1))
        rec["basis"] = [eng.get_basis(int(GEN1[b])) for b in opt]
        vs = np.array([v for v, _ in rec["basis"]], np.int32)
        rec["load_status"] = eng.load_basis(LOADED[opt], vs, vlo[opt], vup[opt])
        rec["loaded"] = _read(eng, LOADED[opt])
        rec["loaded_basis"] = [eng.get_basis(int(LOADED[b])) for b in opt]
        rec["loaded_cert"] = eng.certify(LOADED[opt], vlo[opt], vup[opt])
        # the same bounds from the loaded slots: nothing to do
        rec["again"] = eng.solve_batch(LOADED[opt], OUT_A[opt], vlo[opt], vup[opt])
        rec["again_obj"] = eng.obj(OUT_A[opt])
        # children with other bounds, from the loaded slots and from the original ones
        rec["kids_loaded"] = _solve(eng, LOADED[opt], OUT_A[opt], vlo[perm][opt], vup[perm][opt], retry)
        rec["kids_loaded_obj"] = eng.obj(OUT_A[opt])
        rec["kids_orig"] = _solve(eng, GEN1[opt], OUT_B[opt], vlo[perm][opt], vup[perm][opt], retry)
        rec["kids_orig_obj"] = eng.obj(OUT_B[opt])
        # the original slots rebuilt in place
        rec["rebuild_status"] = eng.rebuild(GEN1[opt])
        rec["rebuild_stats"] = eng.last_rebuild_stats()
        rec["rebuilt"] = _read(eng, GEN1[opt])
        rec["rebuilt_cert"] = eng.certify(GEN1[opt], vlo[opt], vup[opt])
        rec["rebuilt_basis"] = [eng.get_basis(int(GEN1[b])) for b in opt]
        return rec
    finally:
        eng.close()


@pytest.mark.parametrize("shape,arr,form", SOLVED, ids=str)
def test_a_loaded_optimal_basis_needs_no_pivot_and_has_the_same_children(shape, arr, form):
    rec = _solved(shape, arr, form)
    opt = rec["opt"]
    assert len(opt) >= 12 and np.all(rec["load_status"] == 0)
    st, it = rec["again"]
    assert np.all(st == OPTIMAL) and np.all(it == 0), (st, it)
    for k, b in enumerate(opt):
        ref = rec["gen1"]["obj"][b]
        assert abs(rec["again_obj"][k] - ref) <= RTOL * (1.0 + abs(ref)), (shape, arr, form, b)
        assert abs(rec["loaded"]["obj"][k] - ref) <= RTOL * (1.0 + abs(ref)), (shape, arr, form, b)
        assert np.array_equal(rec["loaded_basis"][k][0], rec["basis"][k][0])
    (st_l, _), (st_o, _) = rec["kids_loaded"], rec["kids_orig"]
    assert np.array_equal(st_l, st_o), (st_l, st_o)
    for k in np.nonzero(st_o == OPTIMAL)[0]:
        ref = rec["kids_orig_obj"][k]
        assert abs(rec["kids_loaded_obj"][k] - ref) <= RTOL * (1.0 + abs(ref)), (shape, arr, form, k)


@pytest.mark.parametrize("shape,arr,form", SOLVED, ids=str)
def test_loaded_and_rebuilt_slots_pass_the_certificate(shape, arr, form):
    rec = _solved(shape, arr, form)
    opt = rec["opt"]
    print("loaded:", rec["loaded_cert"]["res"].max(axis=0), "rebuilt:", rec["rebuilt_cert"]["res"].max(axis=0))
    assert np.all(rec["loaded_cert"]["verdict"] == 0), rec["loaded_cert"]
    assert np.all(rec["rebuild_status"] == 0)
    assert rec["rebuild_stats"]["rebuilt"] == len(opt) and rec["rebuild_stats"]["failed"] == 0
    assert np.all(rec["rebuilt_cert"]["verdict"] == 0), rec["rebuilt_cert"]
    for k, b in enumerate(opt):
        # a rebuild keeps the basis, every nonbasic status and value; what it recomputes stays within RTOL
        assert np.array_equal(rec["rebuilt_basis"][k][0], rec["basis"][k][0])
        non = rec["basis"][k][0] != bc.BASIC
        assert np.array_equal(rec["rebuilt"]["prim"][k][non], rec["gen1"]["prim"][b][non])
        for what in ("prim", "dual"):
            _close(rec["rebuilt"][what][k], rec["gen1"][what][b], "%s rebuilt %s" % ((shape, arr, form, int(b)), what))
        _close([rec["rebuilt"]["obj"][k]], [rec["gen1"]["obj"][b]], "%s rebuilt objective" % ((shape, arr, form, int(b)),))


def test_the_revised_rebuild_is_the_refactorisation():
    """bit for bit: two engines make the same solves, one calls bslv_lpq_rebuild, the other bslv_lpq_refactor"""
    s = lc.general_set(33, 257, "a")
    out = []
    for call in ("rebuild", "refactor"):
        eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, "revised")
        try:
            st, _ = _gen1(eng, s, True)
            opt = np.nonzero(st == OPTIMAL)[0]
            status = getattr(eng, call)(GEN1[opt])
            assert np.all(status == 0)
            assert all(eng.slot_age(int(x)) == 0 for x in GEN1[opt])
            heads = [eng.get_inverse(int(x))[1].tobytes() for x in GEN1[opt][:3]]
            out.append((_bits(_read(eng, GEN1[opt])), heads, eng.last_refactor_stats()))
        finally:
            eng.close()
    assert out[0] == out[1]


# ---- 4. across forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 257), (24, 1536)], ids=str)
@pytest.mark.parametrize("src_form,dst_form", [("tableau", "revised"), ("revised", "tableau")])
def test_a_basis_moves_between_the_forms(shape, src_form, dst_form):
    s = lc.general_set(shape[0], shape[1], "a")
    rec = _solved(shape, "a", src_form)
    opt = rec["opt"]
    vs = np.array([v for v, _ in rec["basis"]], np.int32)
    eng = _engine(s["A"], s["lo"], s["up"], s["cost"], s["var_first"], s["var_cnt"], POOL, dst_form)
    try:
        status = eng.load_basis(LOADED[opt], vs, s["vlo"][opt], s["vup"][opt])
        assert np.all(status == 0)
        got = _read(eng, LOADED[opt])
        for k, b in enumerate(opt):
            tag = (shape, src_form, dst_form, int(b))
            _close(got["prim"][k], rec["gen1"]["prim"][b], "%s primal" % (tag,))
            _close(got["dual"][k], rec["gen1"]["dual"][b], "%s dual" % (tag,))
            _close([got["obj"][k]], [rec["gen1"]["obj"][b]], "%s objective" % (tag,))
            assert np.array_equal(eng.get_basis(int(LOADED[b]))[0], vs[k])
        st, it = eng.solve_batch(LOADED[opt], OUT_A[opt], s["vlo"][opt], s["vup"][opt])
        assert np.all(st == OPTIMAL) and np.all(it == 0), (st, it)
        if dst_form == "revised":
            assert all(eng.slot_age(int(x)) == 0 for x in LOADED[opt])
    finally:
        eng.close()


# ---- 7. failures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_a_singular_basis_beside_healthy_ones(form):
    A, lo, up, cost = bc.shape_model(15, 16)
    A2, sing = bc.singular_basis(A, lo, up)
    healthy = bc.bases(("gpu", "singular"), A2, lo, up, cost, 11)
    (_, v1, r1), (_, v2, r2) = healthy[2], healthy[4]
    eng = _engine(A2, lo, up, cost, 0, 0, 5, form)
    try:
        eng.reset_slot(4)
        fresh = (_bits(_read(eng, [4])), eng.get_basis(4))
        status = eng.load_basis([1, 2, 3], np.array([v1, sing, v2], np.int32))
        assert list(status) == [0, UNDEFINED, 0]
        st = eng.last_rebuild_stats()
        assert st["rebuilt"] == 2 and st["failed"] == 1
        got = _read(eng, [1, 2, 3])
        for k, ref in ((0, r1), (2, r2)):
            _close(got["prim"][k], ref[0], "healthy %d primal" % k)
            _close(got["dual"][k], ref[1], "healthy %d dual" % k)
            _close([got["obj"][k]], [ref[2]], "healthy %d objective" % k)
        # the singular one: a reset slot
        assert _bits(_read(eng, [2])) == fresh[0]
        b2 = eng.get_basis(2)
        assert np.array_equal(b2[0], fresh[1][0]) and np.array_equal(b2[1], fresh[1][1])
        assert np.all(b2[0][:15] == bc.BASIC)
        # healthy alone: the same bits as beside the singular one
        assert list(eng.load_basis([4], v1.reshape(1, -1))) == [0]
        assert _bits(_read(eng, [4])) == _bits(_read(eng, [1]))
    finally:
        eng.close()


@pytest.mark.parametrize("form", FORMS)
def test_refused_arguments_change_nothing(form):
    A, lo, up, cost = bc.small_model()
    M, N = A.shape
    good = bc.bases(("gpu", "small-arg"), A, lo, up, cost, 7)[1][1]
    # per-LP bounds on the rows, so that vlo / vup are part of the call
    eng = _engine(A, lo, up, cost, 0, M, 3, form)
    try:
        vlo, vup = lo[:M].reshape(1, M), up[:M].reshape(1, M)
        assert list(eng.load_basis([1], good.reshape(1, -1), vlo, vup)) == [0]
        before = (_bits(_read(eng, [1])), eng.get_basis(1)[0].tobytes(), eng.last_rebuild_stats())

        def bad(k, code):
            v = good.copy()
            v[k] = code
            return v

        nb = int(np.nonzero(good != bc.BASIC)[0][0])
        ba = int(np.nonzero(good == bc.BASIC)[0][0])
        cases = {"code 0": bad(nb, 0), "code 6": bad(nb, 6), "code -1": bad(nb, -1),
                 "one more basic": bad(nb, bc.BASIC), "one fewer basic": bad(ba, bc.LOWER if np.isfinite(lo[ba]) else (bc.UPPER if np.isfinite(up[ba]) else bc.FREE)),
                 "LOWER without a lower bound": bad(0, bc.LOWER),      # row 0: (-inf, 4]
                 "UPPER without an upper bound": bad(M + 0, bc.UPPER),  # column 0: [0, inf)
                 "LOWER on a free variable": bad(M + 2, bc.LOWER), "UPPER on a free variable": bad(M + 2, bc.UPPER),
                 "FREE on a bounded variable": bad(M + 1, bc.FREE), "FREE on a half-bounded variable": bad(M + 0, bc.FREE),
                 "FIXED on a boxed variable": bad(M + 1, bc.FIXED)}
        assert not np.isfinite(lo[0]) and not np.isfinite(up[M]) and np.isinf(lo[M + 2]) and np.isinf(up[M + 2])
        for tag, v in cases.items():
            # (where the changed variable was basic or is made basic the count is off as well: the call is refused either way)
            with pytest.raises(BslvError):
                eng.load_basis([1], v.reshape(1, -1), vlo, vup)
            assert (_bits(_read(eng, [1])), eng.get_basis(1)[0].tobytes()) == before[:2], tag
        for tag, slots in (("slot -1", [-1]), ("slot = pool", [3]), ("named twice", [1, 1])):
            with pytest.raises(BslvError):
                eng.load_basis(slots, np.tile(good, (len(slots), 1)), np.tile(vlo, (len(slots), 1)), np.tile(vup, (len(slots), 1)))
            with pytest.raises(BslvError):
                eng.rebuild(slots)
            assert (_bits(_read(eng, [1])), eng.get_basis(1)[0].tobytes()) == before[:2], tag
        lib = eng.lib
        one = np.array([1], np.int32)
        g = np.ascontiguousarray(good, np.int32)
        lib.bslv_lpq_load_basis.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
        lib.bslv_lpq_rebuild.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        assert lib.bslv_lpq_load_basis(eng.h, -1, one.ctypes.data, g.ctypes.data, None, None, None) == 2
        assert lib.bslv_lpq_load_basis(eng.h, 1, one.ctypes.data, g.ctypes.data, np.ascontiguousarray(vlo).ctypes.data, None, None) == 2
        assert lib.bslv_lpq_rebuild(eng.h, -1, one.ctypes.data, None) == 2
        assert (_bits(_read(eng, [1])), eng.get_basis(1)[0].tobytes()) == before[:2]
        # and the refusals of the tableau form's refactorisation stand
        if form == "tableau":
            with pytest.raises(BslvError):
                eng.refactor([1])
            assert eng.set_refactor(1) == 2 and eng.set_refactor_period(5) == 2
        else:
            assert eng.set_method(1) == 2
    finally:
        eng.close()


# ---- 8. parked slots --------------------------------------------------------------------------------------------------------
def test_a_parked_slot_is_rebuilt_as_a_materialised_one():
    from bensolve_amd import synth
    from bensolve_amd.lp import P2Model
    prob = synth.covering_vlp(30, 15, 3, 5)
    model = P2Model(prob)
    B = 24
    rng = np.random.default_rng(4)
    n = prob["n"]
    X = rng.random((B, n)) * (3.0 / n) + 1.0 / n
    V = (X @ prob["P"].T) * rng.uniform(0.2, 1.2, size=(B, 1)) + rng.normal(scale=0.05, size=(B, prob["q"]))
    dst = np.arange(1, B + 1, dtype=np.int32)
    out = {}
    for how in ("parked", "materialised"):
        eng = LpEngine.from_model(model, pool_slots=B + 2)
        try:
            eng.reset_slot(0)
            st0, _ = eng.solve_batch([0], [0], np.full((1, model.r), -np.inf), model.ub_for(V[:1]))
            assert st0[0] == OPTIMAL
            eng.set_lazy(1)
            st, it = eng.solve_batch(np.zeros(B, np.int32), dst, np.full((B, model.r), -np.inf), model.ub_for(V))
            assert np.all(st == OPTIMAL)
            eng.park(dst)
            eng.discard_pending()
            ps = eng.park_stats()
            assert ps["parked"] >= 1 and ps["live"] == ps["parked"], ps
            if how == "materialised":
                eng.materialise(dst)
                assert eng.park_stats()["live"] == 0
            assert np.all(eng.rebuild(dst) == 0)
            ps2 = eng.park_stats()
            assert ps2["live"] == 0, ps2                           # park_stats[4]: the records are gone
            n_all = model.M + model.N
            out[how] = (eng.obj(dst).tobytes(), eng.primal(dst, 0, n_all).tobytes(), eng.dual(dst, 0, n_all).tobytes(),
                        b"".join(eng.get_basis(int(s))[0].tobytes() for s in dst))
            # the rebuilt slots are parents like any other
            st2, _ = eng.solve_batch(dst, dst, np.full((B, model.r), -np.inf), model.ub_for(V))
            assert np.all(st2 == OPTIMAL)
        finally:
            eng.close()
    assert out["parked"] == out["materialised"]


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        print("digest " + _child_digest())
