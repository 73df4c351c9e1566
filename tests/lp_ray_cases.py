"""The yardstick and the inputs of the ray tests (bslv_lpq_set_rays / bslv_lpq_certify_rays, include/bslv_hip.h).  No GPU in here.

certify_ray     the residuals and the verdict of a Farkas vector or a recession direction, from the model and the vector alone, in
                np.longdouble: the definitions of the header, restated
ray_terms       (L, S) per residual -- the terms of its longest sum and its largest sum of |terms| -- for the bound rule of
                tests/test_lp_certify_gpu.py
boxed_set       one model per shape with every column boxed (no variable ever needs an artificial bound) and 16 LPs that differ in the
                row bounds; LPs 3, 5 and 11 are infeasible by construction with margin 1, and the proof is known
handmade        x1 + x2 >= 3 with 0 <= x <= 1

Run as a program (`python tests/lp_ray_cases.py [M N ...]`) it solves every LP of every boxed set with both CPU yardsticks of
tests/lp_cases.py and checks the constructed proofs: the check made before anything goes to the GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lp_cases as lc
from lp_cases import NLP, OPTIMAL, INFEASIBLE

LD = np.longdouble
NONE, FARKAS, DIRECTION = 0, 1, 2
TOL = (1e-8, 1e-9, 1e-9, 1e-9)          # ident (the certificate's dj), rows, the dual-zero threshold, the margin (its gap, applied the same way)
SHAPES = [(15, 16), (16, 17), (31, 64), (32, 65), (33, 257), (24, 1120), (24, 1121), (24, 2049)]
BAD_LPS = (3, 5, 11)


def full_cost(M, N, cost):
    """a cost over all M + N variables: from the engine's own vector (N + 1, [0] the shift) or as it is"""
    cost = np.asarray(cost, np.float64)
    if len(cost) == N + 1:
        return np.concatenate([np.zeros(M), cost[1:]])
    assert len(cost) == M + N
    return cost


def certify_ray(A, lo, up, cost, kind, vec, tol=None):
    """dict(res (4), at (4), verdict) of one LP; lo / up over rows then columns, vec likewise, cost as full_cost takes it.
    FARKAS     res = ident max_j |z_{M+j} + sum_i a_ij z_i|; open: the largest |z_k| over tol[2] whose needed bound (lo for z > 0, up for
               z < 0) is infinite; S = sum z_k (needed bound) over the other entries over tol[2]; sum |z_k (needed bound)|
    DIRECTION  res = rows max_i |dr_i - sum_j a_ij dx_j|; cross: max of -d_k over the finite lo and of d_k over the finite up, not below
               0; -c . d; sum |c_k d_k|
    verdict: bit 0 res[0] over tol[0] (FARKAS) / tol[1] (DIRECTION), bit 1 res[1] over tol[2], bit 2 not res[2] > tol[3] (1 + res[3]),
    bit 3 kind NONE (res NaN, at -1); a NaN residual sets its bit."""
    tol = TOL if tol is None else tol
    M, N = A.shape
    if kind == NONE:
        return dict(res=np.full(4, np.nan), at=np.full(4, -1), verdict=15)
    vec = np.asarray(vec, np.float64)
    lo, up = np.asarray(lo, np.float64), np.asarray(up, np.float64)
    Al, z = A.astype(LD), vec.astype(LD)
    at = [-1, -1, -1, -1]
    if kind == FARKAS:
        ident = np.abs(z[M:] + Al.T @ z[:M])
        r0, at[0] = ident.max(), M + int(np.argmax(ident))
        nz = np.abs(vec) > tol[2]
        bnd = np.where(vec > 0, lo, up)
        fin = np.isfinite(bnd)
        op = np.where(nz & ~fin, np.abs(vec), 0.0)
        r1 = LD(op.max())
        if r1 > 0:
            at[1] = int(np.argmax(op))
        use = nz & fin
        prod = z[use] * bnd[use].astype(LD)
        r2, r3 = prod.sum(), np.abs(prod).sum()
    else:
        rows = np.abs(z[:M] - Al @ z[M:])
        r0, at[0] = rows.max(), int(np.argmax(rows))
        cr = np.maximum(np.where(np.isfinite(lo), -vec, 0.0), np.where(np.isfinite(up), vec, 0.0))
        r1 = LD(max(cr.max(), 0.0))
        if r1 > 0:
            at[1] = int(np.argmax(cr))
        prod = full_cost(M, N, cost).astype(LD) * z
        r2, r3 = -prod.sum(), np.abs(prod).sum()
    res = np.array([float(r0), float(r1), float(r2), float(r3)])
    if np.isnan(vec).any():
        res[0] = res[1] = np.nan
    verdict = 0
    if not res[0] <= (tol[0] if kind == FARKAS else tol[1]):
        verdict |= 1
    if not res[1] <= tol[2]:
        verdict |= 2
    if not res[2] > tol[3] * (1.0 + res[3]):
        verdict |= 4
    return dict(res=res, at=np.array(at), verdict=verdict)


def ray_terms(A, lo, up, cost, kind, vec, tol=None):
    """per residual (L, S): the number of terms of its longest sum and its largest sum of |terms| (res[1] is a maximum of entries: one
    term, no arithmetic)"""
    tol = TOL if tol is None else tol
    M, N = A.shape
    vec = np.asarray(vec, np.float64)
    absA, a = np.abs(A), np.abs(vec)
    if kind == FARKAS:
        bnd = np.where(vec > 0, lo, up)
        use = (a > tol[2]) & np.isfinite(bnd)
        s = float(np.abs(vec[use] * bnd[use]).sum())
        return [(M + 1, float((a[M:] + absA.T @ a[:M]).max())), (1, 0.0), (M + N, s), (M + N, s)]
    s = float(np.abs(full_cost(M, N, cost) * vec).sum())
    return [(N + 1, float((a[:M] + absA @ a[M:]).max())), (1, 0.0), (M + N, s), (M + N, s)]


def handmade(up2=1.0):
    """x1 + x2 >= 3 with 0 <= x1 <= 1, 0 <= x2 <= up2: (A, lo, up, cost); z = (1, -1, -1) proves it infeasible for up2 = 1"""
    return np.array([[1.0, 1.0]]), np.array([3.0, 0.0, 0.0]), np.array([np.inf, 1.0, up2]), np.zeros(3)


_SETS = {}


def boxed_set(M, N):
    """lp_cases.random_lp's feasible and bounded model of the shape (seed lp_cases.model_seed) with EVERY column of type d and the bounds
    [x0 - 1, x0 + 2]: no variable ever needs an artificial bound.  Arrangement "a": var_first = 0, var_cnt = M, every row per LP.  LP 0
    has the model's bounds, LP t its rows around A x_t for a point x_t of the box, as lp_cases.general_set makes them; the LPs of BAD_LPS
    ask one row i (one with a lower bound by type) for r_i >= max over the box of a_i . x + 1: infeasible with margin 1, proved by
    z = e_i - a_i.  Returns a dict: A, lo, up, cost, var_first, var_cnt, vlo / vup, lps (the full bounds of every LP), perm, and proofs
    (LP -> z)."""
    key = (M, N)
    if key in _SETS:
        return _SETS[key]
    rng = np.random.default_rng(lc.model_seed(M, N))
    A, lo, up, cost, x0, tr, tc = lc.random_lp(M, N, rng, "feasible", bounded=True, parts=True)
    lo, up = lo.copy(), up.copy()
    lo[M:], up[M:] = x0 - 1.0, x0 + 2.0
    clo, cup = lo[M:], up[M:]
    rng = np.random.default_rng(lc.model_seed(M, N) * 1000 + 3)
    vlo, vup = np.tile(lo[:M], (NLP, 1)), np.tile(up[:M], (NLP, 1))
    lower = [i for i in range(M) if tr[i] in "lds"]
    assert len(lower) >= 1, (M, N, tr)
    proofs = {}
    for t in range(1, NLP):
        xt = np.clip(x0 + np.round(rng.normal(size=N) * 0.4 * t), clo, cup)
        vlo[t], vup[t] = lc._typed(tr, A @ xt, rng, 2)
        if t in BAD_LPS:
            i = lower[t % len(lower)]
            top = float(np.where(A[i] > 0, A[i] * cup, A[i] * clo).sum())
            vlo[t, i] = top + 1.0
            if np.isfinite(vup[t, i]):
                vup[t, i] = top + 1.0 if tr[i] == "s" else top + 2.0
            z = np.zeros(M + N)
            z[i], z[M:] = 1.0, -A[i]
            proofs[t] = z
    assert np.array_equal(np.isfinite(vlo), np.tile(np.isfinite(lo[:M]), (NLP, 1)))
    assert np.array_equal(np.isfinite(vup), np.tile(np.isfinite(up[:M]), (NLP, 1)))
    lps = []
    for t in range(NLP):
        l, u = lo.copy(), up.copy()
        l[:M], u[:M] = vlo[t], vup[t]
        lps.append((l, u))
    perm = (np.arange(NLP) * 7 + 3) % NLP
    out = dict(M=M, N=N, A=A, lo=lo, up=up, cost=cost, x0=x0, tr=tr, var_first=0, var_cnt=M, vlo=vlo, vup=vup, lps=lps, perm=perm, proofs=proofs)
    _SETS[key] = out
    return out


_REF = {}


def boxed_references(M, N):
    """(status of the oracle, status of HiGHS) of every LP of a boxed set, computed once and shared"""
    if (M, N) not in _REF:
        s = boxed_set(M, N)
        _REF[(M, N)] = [(lc.oracle_solution(s["A"], l, u, s["cost"])[0], lc.highs(s["A"], l, u, s["cost"])[0]) for l, u in s["lps"]]
    return _REF[(M, N)]


def assert_boxed_references(M, N):
    """what the tests assert of the inputs before they look at the engine: the LPs of BAD_LPS INFEASIBLE and the other 13 OPTIMAL for
    both yardsticks, and the constructed proofs certified with margin 1.  Returns the statuses."""
    s = boxed_set(M, N)
    ref = boxed_references(M, N)
    for t, (so, sh) in enumerate(ref):
        want = INFEASIBLE if t in BAD_LPS else OPTIMAL
        assert so == want and sh == want, (M, N, t, so, sh, want)
    for t in BAD_LPS:
        l, u = s["lps"][t]
        c = certify_ray(s["A"], l, u, s["cost"], FARKAS, s["proofs"][t])
        assert c["verdict"] == 0 and c["res"][0] == 0.0 and c["res"][1] == 0.0 and c["res"][2] == 1.0, (M, N, t, c)
    return np.array([r[0] for r in ref])


if __name__ == "__main__":
    v = [int(a) for a in sys.argv[1:]]
    for M, N in (list(zip(v[0::2], v[1::2])) if v else SHAPES):
        st = assert_boxed_references(M, N)
        print("lp_ray_cases boxed set M %d N %d statuses %s" % (M, N, "".join(str(x) for x in st)), flush=True)
