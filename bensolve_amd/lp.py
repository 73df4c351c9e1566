"""Host-side mirror of the reference's scalar-LP interface for the hot path.

`P2Model` builds the LP  (P_2(v))  of bslv_algs.c:562-664 (init_P2) in GLPK's row/column
model; `LpEngine` is a thin ctypes view of the batched engine of include/bslv_hip.h section 1.
"""
import ctypes
import numpy as np
from ._lib import load_library, check

INF = float("inf")


def bounds_from_types(types, lb, ub):
    """'f','l','u','d','s' (bslv_lists.h:41-48, bslv_lp.c:34-43) -> (lo, up) arrays."""
    types = np.asarray(types)
    t = np.array([chr(c) if not isinstance(c, str) else c for c in types])
    lo = np.where(np.isin(t, ["l", "d", "s"]), lb, -INF).astype(np.float64)
    up = np.where(np.isin(t, ["u", "d"]), ub, INF).astype(np.float64)
    up = np.where(t == "s", lb, up)
    return lo, up


class P2Model:
    """min z  s.t.  vlp rows/cols,  -P x + y = 0,  R_j.y - z <= ub_j (j<r),  eta.y free.

    Index map (0-based variable ids; aux = rows, structural = cols), Appendix C.2 of SURVEY.md:
      rows 0..m-1 : A x             cols 0..n-1   : x
      rows m..m+q-1 : -P x + y = 0  cols n..n+q-1 : y (free)
      rows m+q..m+q+r-1 : R_j.y - z cols n+q      : z (free, cost 1)
      row  m+q+r : eta.y (free in the inhomogeneous problem)
    `R` is q x r with generators as COLUMNS (ZR[j*p+i], bslv_algs.c:599)."""

    def __init__(self, prob, R=None, eta=None):
        m, n, q = prob["m"], prob["n"], prob["q"]
        A, P = np.asarray(prob["A"], np.float64), np.asarray(prob["P"], np.float64)
        if R is None:
            R = np.eye(q)      # default cone, c = (1..1): Z = I scaled so Z'c = 1 (bslv_vlp.c:661-672,775-792)
        R = np.asarray(R, np.float64)
        r = R.shape[1]
        M, N = m + q + r + 1, n + q + 1
        L = np.zeros((M, N))
        L[:m, :n] = A
        L[m:m + q, :n] = -P
        L[m:m + q, n:n + q] = np.eye(q)
        L[m + q:m + q + r, n:n + q] = R.T
        L[m + q:m + q + r, n + q] = -1.0
        if eta is not None:
            L[m + q + r, n:n + q] = eta
        rlo, rup = bounds_from_types(prob["rtype"], prob["rlb"], prob["rub"])
        clo, cup = bounds_from_types(prob["ctype"], prob["clb"], prob["cub"])
        lo = np.concatenate([rlo, np.zeros(q), np.full(r, -INF), [-INF], clo, np.full(q + 1, -INF)])
        up = np.concatenate([rup, np.zeros(q), np.zeros(r), [INF], cup, np.full(q + 1, INF)])
        cost = np.zeros(N + 1)
        cost[N] = 1.0
        self.m, self.n, self.q, self.r, self.M, self.N = m, n, q, r, M, N
        self.L, self.lo, self.up, self.cost, self.R = L, lo, up, cost, R
        self.var_first = m + q        # aux variables of the r rows
        self.w_first = m              # duals of rows m..m+q-1  (bslv_algs.c:1050)
        self.y_first = M + n          # primals of cols n..n+q-1 (bslv_algs.c:1055)

    def ub_for(self, V):
        """rows->ub[j] = R_j . v (bslv_algs.c:1041-1046); V is B x q."""
        return np.asarray(V, np.float64) @ self.R


class LpEngine:
    def __init__(self, M, N, A, lo, up, cost, var_first, var_cnt, pool_slots):
        self.lib = load_library()
        self.M, self.N, self.vcnt = M, N, var_cnt
        A = np.ascontiguousarray(A, np.float64)
        lo = np.ascontiguousarray(lo, np.float64)
        up = np.ascontiguousarray(up, np.float64)
        cost = np.ascontiguousarray(cost, np.float64)
        assert A.shape == (M, N) and lo.shape == (M + N,) and up.shape == (M + N,) and cost.shape == (N + 1,)
        h = ctypes.c_void_p()
        check(self.lib.bslv_lpq_create(ctypes.byref(h), M, N, A.ctypes.data, lo.ctypes.data, up.ctypes.data,
                                       cost.ctypes.data, var_first, var_cnt, pool_slots))
        self.h = h
        self.pool_slots = pool_slots

    @classmethod
    def from_model(cls, model, pool_slots):
        return cls(model.M, model.N, model.L, model.lo, model.up, model.cost, model.var_first, model.r, pool_slots)

    def close(self):
        if getattr(self, "h", None):
            self.lib.bslv_lpq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slot_bytes(self):
        return self.lib.bslv_lpq_slot_bytes(self.h)

    def set_profile(self, on):
        check(self.lib.bslv_lpq_set_profile(self.h, int(on)))

    def reset_slot(self, slot):
        check(self.lib.bslv_lpq_reset_slot(self.h, slot))

    def rows_folded(self):
        import ctypes
        self.lib.bslv_lpq_rows_folded.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_rows_folded(self.h))

    def set_lazy(self, on):
        import ctypes
        self.lib.bslv_lpq_set_lazy.argtypes = [ctypes.c_void_p, ctypes.c_int]
        check(self.lib.bslv_lpq_set_lazy(self.h, int(on)))

    def materialise(self, slots):
        import ctypes
        slots = np.ascontiguousarray(slots, np.int32)
        self.lib.bslv_lpq_materialise.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_materialise(self.h, len(slots), slots.ctypes.data))

    def discard_pending(self):
        import ctypes
        self.lib.bslv_lpq_discard_pending.argtypes = [ctypes.c_void_p]
        check(self.lib.bslv_lpq_discard_pending(self.h))

    def lazy_stats(self):
        import ctypes
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_lazy_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_lazy_stats(self.h, o))
        return dict(skipped=int(o[0]), on_request=int(o[1]), ms=o[2] / 1000.0)

    def park(self, slots):
        """in place of materialise: the slots keep what their tableau pass needs, the engine makes it when they are used (bslv_lpq_park)"""
        slots = np.ascontiguousarray(slots, np.int32)
        self.lib.bslv_lpq_park.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_park(self.h, len(slots), slots.ctypes.data))

    def drop_parked(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        self.lib.bslv_lpq_drop_parked.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_drop_parked(self.h, len(slots), slots.ctypes.data))

    def set_park(self, on):
        self.lib.bslv_lpq_set_park.argtypes = [ctypes.c_void_p, ctypes.c_int]
        check(self.lib.bslv_lpq_set_park(self.h, int(bool(on))))

    def park_stats(self):
        o = (ctypes.c_long * 5)()
        self.lib.bslv_lpq_park_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_park_stats(self.h, o))
        return dict(zip(("parked", "for_child", "forced", "dropped", "live"), [int(v) for v in o]))

    def set_bounds(self, lo, up):
        lo = np.ascontiguousarray(lo, np.float64)
        up = np.ascontiguousarray(up, np.float64)
        check(self.lib.bslv_lpq_set_bounds(self.h, lo.ctypes.data, up.ctypes.data))

    def solve_batch(self, src, dst, vlo, vup):
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        vlo = np.ascontiguousarray(vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        check(self.lib.bslv_lpq_solve_batch(self.h, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data,
                                            vup.ctypes.data, status.ctypes.data, iters.ctypes.data))
        return status, iters

    def solve_batch_method(self, method, src, dst, vlo, vup):
        """solve_batch under `method` (0 dual, 1 primal, 2 repair) for this call only; the engine's own method stays what it is.  In the
        revised form the only way to PRIMAL and REPAIR (bslv_lpq_solve_batch_method)."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        vlo = np.ascontiguousarray(vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_method.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        self.lib.bslv_lpq_solve_batch_method.restype = ctypes.c_int
        check(self.lib.bslv_lpq_solve_batch_method(self.h, int(method), B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data,
                                                   vup.ctypes.data, status.ctypes.data, iters.ctypes.data))
        return status, iters

    def solve_batch_method_priced(self, method, dual_rule, primal_rule, src, dst, vlo, vup):
        """solve_batch under `method` (0 dual, 1 primal, 2 repair), the dual pricing rule `dual_rule` and the primal pricing rule
        `primal_rule` (0 dantzig, 1 devex) for this call only; the engine's method and its two pricing switches stay what they are.  In
        the revised form the only way to Devex pricing for a PRIMAL / REPAIR batch (bslv_lpq_solve_batch_method_priced)."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        vlo = np.ascontiguousarray(vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_method_priced.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 6
        self.lib.bslv_lpq_solve_batch_method_priced.restype = ctypes.c_int
        check(self.lib.bslv_lpq_solve_batch_method_priced(self.h, int(method), int(dual_rule), int(primal_rule), B, src.ctypes.data,
                                                          dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data, status.ctypes.data,
                                                          iters.ctypes.data))
        return status, iters

    def solve_batch_canonical(self, dir, src, dst, vlo, vup):
        """solve_batch followed by the tie phase towards the canonical optimal basis for `dir` (var_cnt values), for this call only; the
        engine's own switch and direction stay what they are.  Works in both forms; in the revised form the only way to the tie phase
        (bslv_lpq_solve_batch_canonical).  dir=None hands the library a null pointer (its BSLV_E_ARG raises BslvError, like a NaN)."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        d = None if dir is None else np.ascontiguousarray(dir, np.float64).reshape(self.vcnt)
        vlo = np.ascontiguousarray(vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_canonical.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6
        self.lib.bslv_lpq_solve_batch_canonical.restype = ctypes.c_int
        check(self.lib.bslv_lpq_solve_batch_canonical(self.h, None if d is None else d.ctypes.data, B, src.ctypes.data, dst.ctypes.data,
                                                      vlo.ctypes.data, vup.ctypes.data, status.ctypes.data, iters.ctypes.data))
        return status, iters

    def solve_batch_obj(self, src, dst, cost_first, costs, vlo=None, vup=None):
        """LPs that differ in the objective: costs[b, t] on variable cost_first + t (bslv_lpq_solve_batch_obj)."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        costs = np.ascontiguousarray(costs, np.float64).reshape(B, -1)
        vlo = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vlo is None else vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vup is None else vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_obj.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
        check(self.lib.bslv_lpq_solve_batch_obj(self.h, B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data,
                                                cost_first, costs.shape[1], costs.ctypes.data, status.ctypes.data, iters.ctypes.data))
        return status, iters

    def solve_batch_obj_method(self, method, src, dst, cost_first, costs, vlo=None, vup=None):
        """solve_batch_obj under a simplex method for this call only (bslv_lpq_solve_batch_obj_method): method 1 (primal) is solve_batch_obj,
        0 (dual) makes the parent's basis dual feasible for the new objective and runs dual simplex steps, 2 (repair) does so for
        the LPs where that is possible and starts the others as PRIMAL does.  Both forms; the engine's own method stays what it is."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        costs = np.ascontiguousarray(costs, np.float64).reshape(B, -1)
        vlo = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vlo is None else vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vup is None else vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_obj_method.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
        self.lib.bslv_lpq_solve_batch_obj_method.restype = ctypes.c_int
        check(self.lib.bslv_lpq_solve_batch_obj_method(self.h, int(method), B, src.ctypes.data, dst.ctypes.data, vlo.ctypes.data, vup.ctypes.data,
                                                       int(cost_first), costs.shape[1], costs.ctypes.data, status.ctypes.data, iters.ctypes.data))
        return status, iters

    def last_obj_method_stats(self):
        """of the last solve call (bslv_lpq_last_obj_method_stats): LPs that started dual, nonbasic variables moved at the start, LPs
        REPAIR handed to the primal start, dual pivots"""
        out = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_obj_method_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.bslv_lpq_last_obj_method_stats.restype = ctypes.c_int
        check(self.lib.bslv_lpq_last_obj_method_stats(self.h, out))
        return [int(v) for v in out]

    def solve_batch_obj_canonical(self, ddir, src, dst, cost_first, costs, vlo=None, vup=None):
        """solve_batch_obj followed by the tie phase towards the canonical optimal point for `ddir` (one value per variable of the cost
        range cost_first .. cost_first + costs.shape[1] - 1), for this call only; the engine's own switch, range and direction stay what
        they are.  Works in both forms; in the revised form the only way to the phase (bslv_lpq_solve_batch_obj_canonical).  ddir=None
        hands the library a null pointer (its BSLV_E_ARG raises BslvError, like a NaN or a bad range)."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.ascontiguousarray(dst, np.int32)
        B = len(src)
        costs = np.ascontiguousarray(costs, np.float64).reshape(B, -1)
        d = None if ddir is None else np.ascontiguousarray(ddir, np.float64).reshape(costs.shape[1])
        vlo = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vlo is None else vlo, np.float64).reshape(B, self.vcnt)
        vup = np.ascontiguousarray(np.zeros((B, self.vcnt)) if vup is None else vup, np.float64).reshape(B, self.vcnt)
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        self.lib.bslv_lpq_solve_batch_obj_canonical.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
        self.lib.bslv_lpq_solve_batch_obj_canonical.restype = ctypes.c_int
        check(self.lib.bslv_lpq_solve_batch_obj_canonical(self.h, None if d is None else d.ctypes.data, B, src.ctypes.data, dst.ctypes.data,
                                                          vlo.ctypes.data, vup.ctypes.data, int(cost_first), costs.shape[1], costs.ctypes.data,
                                                          status.ctypes.data, iters.ctypes.data))
        return status, iters

    def _get(self, fn, slots, first, cnt):
        slots = np.ascontiguousarray(slots, np.int32)
        out = np.empty((len(slots), cnt), np.float64)
        check(fn(self.h, len(slots), slots.ctypes.data, first, cnt, out.ctypes.data))
        return out

    def primal(self, slots, first, cnt):
        return self._get(self.lib.bslv_lpq_get_primal, slots, first, cnt)

    def dual(self, slots, first, cnt):
        return self._get(self.lib.bslv_lpq_get_dual, slots, first, cnt)

    def obj(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        out = np.empty(len(slots), np.float64)
        check(self.lib.bslv_lpq_get_obj(self.h, len(slots), slots.ctypes.data, out.ctypes.data))
        return out

    def certify(self, slots, vlo=None, vup=None, cost_first=0, costs=None, tol=None):
        """the optimality certificate of solved slots, computed on the device (bslv_lpq_certify, include/bslv_hip.h): a dict with res
        (B, 5: rows, feas, dj, side, gap), at (B, 5: the variable of the worst residual, -1 where there is none) and verdict (B, a bit
        per kind over its tolerance, 0 = certified).  vlo / vup: the per-LP bounds the LPs were solved with; costs (B, cost_cnt) from
        cost_first: an objective batch's; tol: six values, entries <= 0 or None = the defaults."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        B = len(slots)
        keep = []

        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            keep.append(a)
            return a.ctypes.data

        c = None if costs is None else np.ascontiguousarray(costs, np.float64).reshape(B, -1)
        t = None if tol is None else np.ascontiguousarray(tol, np.float64).reshape(6)
        res, at, verdict = np.zeros((B, 5), np.float64), np.full((B, 5), -1, np.int32), np.zeros(B, np.int32)
        self.lib.bslv_lpq_certify.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        check(self.lib.bslv_lpq_certify(self.h, B, slots.ctypes.data, arr(vlo), arr(vup), int(cost_first), 0 if c is None else c.shape[1], arr(c), arr(t),
                                        res.ctypes.data, at.ctypes.data, verdict.ctypes.data))
        return dict(res=res, at=at, verdict=verdict)

    def last_certify_stats(self):
        """of the last certify call (bslv_lpq_last_certify_stats)"""
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_certify_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_certify_stats(self.h, o))
        return dict(lps=int(o[0]), not_certified=int(o[1]), launches=int(o[2]))

    def set_rays(self, on):
        """the ray store: a kind and a vector per slot for LPs that come back INFEASIBLE or UNBOUNDED (bslv_lpq_set_rays,
        include/bslv_hip.h).  Returns the library's code."""
        self.lib.bslv_lpq_set_rays.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_rays(self.h, int(bool(on))))

    def get_rays(self):
        self.lib.bslv_lpq_get_rays.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_rays(self.h))

    def get_ray(self, slots, vectors=True):
        """(kind (B), ray (B, M + N) or None) of the slots, in the indices of the model as given (bslv_lpq_get_ray): kind 0 none,
        1 a Farkas vector, 2 a recession direction"""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        B = len(slots)
        kind = np.zeros(B, np.int32)
        ray = np.zeros((B, self.M + self.N), np.float64) if vectors else None
        self.lib.bslv_lpq_get_ray.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
        check(self.lib.bslv_lpq_get_ray(self.h, B, slots.ctypes.data, kind.ctypes.data, ray.ctypes.data if vectors else None))
        return kind, ray

    def last_ray_stats(self):
        """of the last solve call (bslv_lpq_last_ray_stats)"""
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_ray_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_ray_stats(self.h, o))
        return dict(farkas=int(o[0]), direction=int(o[1]), none=int(o[2]))

    def certify_rays(self, slots, vlo=None, vup=None, cost_first=0, costs=None, tol=None):
        """the certificate of the stored rays, computed on the device (bslv_lpq_certify_rays, include/bslv_hip.h): a dict with res
        (B, 4: ident / rows, open / cross, margin, its scale), at (B, 4) and verdict (B; 0 = the LP is infeasible / unbounded in the
        model as given).  vlo / vup, cost_first / costs as for certify; tol: four values, entries <= 0 or None = the defaults."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        B = len(slots)
        keep = []

        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            keep.append(a)
            return a.ctypes.data

        c = None if costs is None else np.ascontiguousarray(costs, np.float64).reshape(B, -1)
        t = None if tol is None else np.ascontiguousarray(tol, np.float64).reshape(4)
        res, at, verdict = np.zeros((B, 4), np.float64), np.full((B, 4), -1, np.int32), np.zeros(B, np.int32)
        self.lib.bslv_lpq_certify_rays.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        check(self.lib.bslv_lpq_certify_rays(self.h, B, slots.ctypes.data, arr(vlo), arr(vup), int(cost_first), 0 if c is None else c.shape[1], arr(c), arr(t),
                                             res.ctypes.data, at.ctypes.data, verdict.ctypes.data))
        return dict(res=res, at=at, verdict=verdict)

    def last_ray_certify_stats(self):
        """of the last certify_rays call (bslv_lpq_last_ray_certify_stats)"""
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_ray_certify_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_ray_certify_stats(self.h, o))
        return dict(lps=int(o[0]), not_certified=int(o[1]), launches=int(o[2]))

    def debug_poke(self, slot, what, var, delta):
        """tests only: add delta to the stored value (what 0) or the stored reduced cost (what 1, nonbasic only) of a variable of a
        slot (bslv_lpq_debug_poke).  Returns the library's code (0, or BSLV_E_ARG)."""
        self.lib.bslv_lpq_debug_poke.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
        return int(self.lib.bslv_lpq_debug_poke(self.h, int(slot), int(what), int(var), float(delta)))

    def set_extended(self, on):
        """the extended selection (perturbation, primal clean-up) for every later solve of this engine (include/bslv_hip.h)"""
        self.lib.bslv_lpq_set_extended.argtypes = [ctypes.c_void_p, ctypes.c_int]
        check(self.lib.bslv_lpq_set_extended(self.h, int(bool(on))))

    def set_method(self, m):
        """the simplex method of every later solve_batch: 0 dual (default), 1 primal with a phase 1, 2 dual with a primal start
        for the LPs the dual simplex cannot start (bslv_lpq_set_method, include/bslv_hip.h).  Returns the library's code (0, or
        BSLV_E_ARG for an unknown method or the revised form)."""
        self.lib.bslv_lpq_set_method.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_method(self.h, int(m)))

    def get_method(self):
        self.lib.bslv_lpq_get_method.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_method(self.h))

    def set_pricing(self, rule):
        """the pricing rule of the dual steps of every later solve_batch: 0 largest violation (default), 1 dual Devex
        (bslv_lpq_set_pricing, include/bslv_hip.h).  Returns the library's code (0, or BSLV_E_ARG for an unknown rule)."""
        self.lib.bslv_lpq_set_pricing.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_pricing(self.h, int(rule)))

    def get_pricing(self):
        self.lib.bslv_lpq_get_pricing.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_pricing(self.h))

    def last_pricing_stats(self):
        """Devex pricing of the last solve call (bslv_lpq_last_pricing_stats)"""
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_pricing_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_pricing_stats(self.h, o))
        return dict(weighted=int(o[0]), other_row=int(o[1]), resets=int(o[2]))

    def last_pricing_norms(self, b):
        """tests: the Devex reference norms of the rows of LP b of the last batch, in the engine's own row numbering
        (bslv_lpq_last_pricing_norms; raises on BSLV_E_STATE when the last solve call did not run under Devex)"""
        M = self.M - self.rows_folded()
        s = np.empty(M, np.float64)
        self.lib.bslv_lpq_last_pricing_norms.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_pricing_norms(self.h, int(b), s.ctypes.data))
        return s

    def set_primal_pricing(self, rule):
        """the pricing rule of the primal steps (objective batches; PRIMAL / REPAIR batches while the dual rule is the default):
        0 largest reduced-cost violation (default), 1 primal Devex (bslv_lpq_set_primal_pricing, include/bslv_hip.h).  Returns the
        library's code (0, or BSLV_E_ARG for an unknown rule)."""
        self.lib.bslv_lpq_set_primal_pricing.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_primal_pricing(self.h, int(rule)))

    def get_primal_pricing(self):
        self.lib.bslv_lpq_get_primal_pricing.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_primal_pricing(self.h))

    def last_primal_pricing_stats(self):
        """primal Devex pricing of the last solve call (bslv_lpq_last_primal_pricing_stats)"""
        o = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_primal_pricing_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_primal_pricing_stats(self.h, o))
        return dict(weighted=int(o[0]), other_col=int(o[1]), resets=int(o[2]))

    def last_primal_pricing_norms(self, b):
        """tests: the primal Devex reference norms of LP b of the last batch by variable of the engine's own model, rows (less the
        folded ones) then columns; 0 for a basic variable (bslv_lpq_last_primal_pricing_norms; raises on BSLV_E_STATE when the
        last solve call ran no weighted instance)"""
        t = np.empty(self.M - self.rows_folded() + self.N, np.float64)
        self.lib.bslv_lpq_last_primal_pricing_norms.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_primal_pricing_norms(self.h, int(b), t.ctypes.data))
        return t

    def set_canonical(self, on, dir=None):
        """canonical optimal duals for every later solve_batch: the basis that stays optimal when the per-LP bounds move by
        t * dir (var_cnt values) for small t > 0, found by a tie phase after optimality (bslv_lpq_set_canonical, include/bslv_hip.h).
        Returns the library's code (0, or BSLV_E_ARG for the revised form or a missing direction)."""
        self.lib.bslv_lpq_set_canonical.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        d = None if dir is None else np.ascontiguousarray(dir, np.float64)
        if on and d is not None and getattr(self, "vcnt", None) is not None:      # (a borrowed view of a driver's engine does not know its range)
            assert d.shape == (self.vcnt,)
        return int(self.lib.bslv_lpq_set_canonical(self.h, int(bool(on)), None if d is None else d.ctypes.data))

    def get_canonical(self):
        self.lib.bslv_lpq_get_canonical.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_canonical(self.h))

    def last_canonical_stats(self):
        """tie phase of the last solve_batch (bslv_lpq_last_canonical_stats)"""
        o = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_canonical_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_canonical_stats(self.h, o))
        return dict(entered=int(o[0]), tie_pivots=int(o[1]), no_candidate=int(o[2]), capped=int(o[3]))

    def set_canonical_obj(self, on, cost_first=None, ddir=None):
        """canonical optimal points for every later solve_batch_obj over the cost range cost_first .. cost_first + len(ddir) - 1:
        the solution that stays optimal for the costs c + t * ddir for small t > 0, found by a tie phase after optimality
        (bslv_lpq_set_canonical_obj, include/bslv_hip.h).  Returns the library's code (0, or BSLV_E_ARG for the revised form, a
        bad range, a missing or non-finite direction)."""
        self.lib.bslv_lpq_set_canonical_obj.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        d = None if ddir is None else np.ascontiguousarray(ddir, np.float64).reshape(-1)
        return int(self.lib.bslv_lpq_set_canonical_obj(self.h, int(bool(on)), 0 if cost_first is None else int(cost_first),
                                                       0 if d is None else len(d), None if d is None else d.ctypes.data))

    def get_canonical_obj(self):
        self.lib.bslv_lpq_get_canonical_obj.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_canonical_obj(self.h))

    def last_canonical_obj_stats(self):
        """tie phase of the last solve_batch_obj (bslv_lpq_last_canonical_obj_stats)"""
        o = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_canonical_obj_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_canonical_obj_stats(self.h, o))
        return dict(entered=int(o[0]), tie_iters=int(o[1]), unbounded=int(o[2]), capped=int(o[3]))

    def refactor(self, slots):
        """revised form: rebuild the basis inverse of the slots in place from their heads (bslv_lpq_refactor); returns the
        per-slot statuses (0, or 3 = UNDEFINED for a singular basis: the slot is then reset to the standard basis)"""
        slots = np.ascontiguousarray(slots, np.int32)
        st = np.empty(len(slots), np.int32)
        self.lib.bslv_lpq_refactor.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_refactor(self.h, len(slots), slots.ctypes.data, st.ctypes.data))
        return st

    def set_refactor(self, on):
        """the in-call rescue of LPs the pivot cross-check gives up (bslv_lpq_set_refactor).  Returns the library's code (0, or
        BSLV_E_ARG for the tableau form)."""
        self.lib.bslv_lpq_set_refactor.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_refactor(self.h, int(bool(on))))

    def get_refactor(self):
        self.lib.bslv_lpq_get_refactor.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_refactor(self.h))

    def last_refactor_stats(self):
        """of the last solve call or explicit refactor (bslv_lpq_last_refactor_stats)"""
        o = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_refactor_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_refactor_stats(self.h, o))
        return dict(refactorised=int(o[0]), replay_pivots=int(o[1]), rescued=int(o[2]), failed=int(o[3]))

    def set_refactor_period(self, pivots):
        """revised form: refactorise an LP's basis inverse inside a solve once it is `pivots` rank-1 steps old, 0 = off
        (bslv_lpq_set_refactor_period).  Returns the library's code (0, or BSLV_E_ARG for a negative period or the tableau form)."""
        self.lib.bslv_lpq_set_refactor_period.argtypes = [ctypes.c_void_p, ctypes.c_int]
        return int(self.lib.bslv_lpq_set_refactor_period(self.h, int(pivots)))

    def get_refactor_period(self):
        self.lib.bslv_lpq_get_refactor_period.argtypes = [ctypes.c_void_p]
        return int(self.lib.bslv_lpq_get_refactor_period(self.h))

    def slot_age(self, slot):
        """rank-1 steps applied to the slot's basis inverse since it was last built from the identity (bslv_lpq_slot_age; tableau form: 0)"""
        a = ctypes.c_long()
        self.lib.bslv_lpq_slot_age.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        check(self.lib.bslv_lpq_slot_age(self.h, int(slot), ctypes.byref(a)))
        return int(a.value)

    def last_period_stats(self):
        """periodic refactorisation of the last solve call (bslv_lpq_last_period_stats)"""
        o = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_period_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_period_stats(self.h, o))
        return dict(at_start=int(o[0]), in_rounds=int(o[1]), replay_pivots=int(o[2]), max_age=int(o[3]))

    def get_inverse(self, slot, matrix=True):
        """revised form: (basis heads, stored matrix M x M or None) of a slot, in the engine's own indices (bslv_lpq_get_inverse)"""
        self.lib.bslv_lpq_is_revised.argtypes = [ctypes.c_void_p]
        self.lib.bslv_lpq_rows_folded.argtypes = [ctypes.c_void_p]
        M = self.M - int(self.lib.bslv_lpq_rows_folded(self.h))
        heads = np.empty(M, np.int32)
        X = np.empty((M, M), np.float64) if matrix else None
        self.lib.bslv_lpq_get_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_get_inverse(self.h, int(slot), heads.ctypes.data, X.ctypes.data if matrix else None))
        return heads, X

    # status codes of get_basis / load_basis (GLPK's GLP_BS .. GLP_NS)
    VS_BASIC, VS_LOWER, VS_UPPER, VS_FREE, VS_FIXED = 1, 2, 3, 4, 5

    def _own_rows(self):
        self.lib.bslv_lpq_rows_folded.argtypes = [ctypes.c_void_p]
        return self.M - int(self.lib.bslv_lpq_rows_folded(self.h))

    def var_map(self):
        """own_of_given: for every variable of the model as given (rows, then columns) its index in the engine's own model, -1 for a
        row the presolve folded into a column's bounds (bslv_lpq_var_map)"""
        out = np.empty(self.M + self.N, np.int32)
        self.lib.bslv_lpq_var_map.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_var_map(self.h, out.ctypes.data))
        return out

    def get_basis(self, slot):
        """(vstat, row_of) of a slot over the engine's own variables: the status codes VS_*, and the row of every basic variable, -1
        for a nonbasic one (bslv_lpq_get_basis)"""
        n = self._own_rows() + self.N
        vstat, row_of = np.empty(n, np.int32), np.empty(n, np.int32)
        self.lib.bslv_lpq_get_basis.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_get_basis(self.h, int(slot), vstat.ctypes.data, row_of.ctypes.data))
        return vstat, row_of

    def load_basis(self, slots, vstat, vlo=None, vup=None):
        """install the bases vstat (len(slots) x (M + N) codes VS_*, the engine's own model) in the slots; vlo / vup: the per-LP bounds
        the nonbasic values come from, or None for the model's (bslv_lpq_load_basis).  Returns the per-slot statuses: 0, or 3 =
        UNDEFINED for a singular basis (that slot is then reset to the standard basis).  A refused argument raises."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(slots)
        vstat = np.ascontiguousarray(vstat, np.int32).reshape(n, self._own_rows() + self.N)
        assert (vlo is None) == (vup is None)
        if vlo is not None:
            vlo = np.ascontiguousarray(vlo, np.float64).reshape(n, self.vcnt)
            vup = np.ascontiguousarray(vup, np.float64).reshape(n, self.vcnt)
        st = np.zeros(n, np.int32)
        self.lib.bslv_lpq_load_basis.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
        check(self.lib.bslv_lpq_load_basis(self.h, n, slots.ctypes.data, vstat.ctypes.data, None if vlo is None else vlo.ctypes.data,
                                           None if vup is None else vup.ctypes.data, st.ctypes.data))
        return st

    def rebuild(self, slots):
        """rebuild the slots in place from their own basis and the model: every variable keeps its nonbasic status and value
        (bslv_lpq_rebuild; the revised form: bslv_lpq_refactor).  Returns the per-slot statuses as load_basis does."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        st = np.zeros(len(slots), np.int32)
        self.lib.bslv_lpq_rebuild.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_rebuild(self.h, len(slots), slots.ctypes.data, st.ctypes.data))
        return st

    def last_rebuild_stats(self):
        """of the last load_basis / rebuild (bslv_lpq_last_rebuild_stats)"""
        o = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_rebuild_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_lpq_last_rebuild_stats(self.h, o))
        return dict(rebuilt=int(o[0]), replay_pivots=int(o[1]), passes=int(o[2]), failed=int(o[3]))

    def debug_perturb_inverse(self, slot, rel):
        """tests only: a deterministic stand-in for drift in the stored inverse of a slot (bslv_lpq_debug_perturb_inverse)"""
        self.lib.bslv_lpq_debug_perturb_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
        check(self.lib.bslv_lpq_debug_perturb_inverse(self.h, int(slot), float(rel)))

    def debug_swap_heads(self, slot, r, q):
        """tests only: the basic variable of row r and the nonbasic variable at position q of a slot change places in its heads; the
        stored matrix stays the old basis' until refactor (bslv_lpq_debug_swap_heads)"""
        self.lib.bslv_lpq_debug_swap_heads.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        check(self.lib.bslv_lpq_debug_swap_heads(self.h, int(slot), int(r), int(q)))

    def last_stats(self):
        it = ctypes.c_int()
        piv = ctypes.c_long()
        ums = ctypes.c_double()
        tms = ctypes.c_double()
        check(self.lib.bslv_lpq_last_stats(self.h, ctypes.byref(it), ctypes.byref(piv), ctypes.byref(ums), ctypes.byref(tms)))
        ext = (ctypes.c_long * 4)()
        self.lib.bslv_lpq_last_ext_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.bslv_lpq_last_ext_stats(self.h, ext)
        self.lib.bslv_lpq_last_passes.restype = ctypes.c_long
        self.lib.bslv_lpq_last_passes.argtypes = [ctypes.c_void_p]
        self.lib.bslv_lpq_last_launches.restype = ctypes.c_long
        self.lib.bslv_lpq_last_launches.argtypes = [ctypes.c_void_p]
        self.lib.bslv_lpq_last_flip_updates.restype = ctypes.c_long
        self.lib.bslv_lpq_last_flip_updates.argtypes = [ctypes.c_void_p]
        self.lib.bslv_lpq_last_init_chunks.restype = ctypes.c_long
        self.lib.bslv_lpq_last_init_chunks.argtypes = [ctypes.c_void_p]
        p1 = (ctypes.c_long * 3)()
        self.lib.bslv_lpq_last_phase1_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.bslv_lpq_last_phase1_stats(self.h, p1)
        return dict(phase1_lps=int(p1[0]), phase1_iterations=int(p1[1]), phase1_rebuilds=int(p1[2]), init_chunks=self.lib.bslv_lpq_last_init_chunks(self.h), lockstep_iters=it.value, pivots=piv.value, update_ms=ums.value, total_ms=tms.value, passes=self.lib.bslv_lpq_last_passes(self.h), launches=self.lib.bslv_lpq_last_launches(self.h),
                    flip_iterations=ext[0], perturbations=ext[1], primal_steps=ext[2], wrong_sign_removals=ext[3],
                    flip_vector_updates=self.lib.bslv_lpq_last_flip_updates(self.h))
