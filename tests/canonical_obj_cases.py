"""Cases for the canonical-point tests (tests/test_lp_canonical_obj_capi.py, tests/test_lp_canonical_obj_gpu.py,
tests/test_dual_variant_canonical_gpu.py): problems, weights w that are normal to faces of dimension >= 1 of the upper image, and the
EXPECTED canonical optimal point y of P1(w) from scipy's HiGHS -- nothing here touches the GPU or oracle/.

The canonical optimal point of P1(w): min w.y, y = P x, x feasible, for a direction ddir is the optimal y that stays optimal for the
weights w + t ddir for all small t > 0 (include/bslv_hip.h, bslv_lpq_set_canonical_obj).  HiGHS knows no such rule, but it can solve
the LPs with the shifted weights: y(t) is piecewise constant in t, so a y that is the minimiser at t1 = 2^-10 AND at t2 = 2^-11 and
is still optimal at t = 0 is the vertex of the image that is optimal on all of (0, t1] -- the keep rule of canonical_cases.py,
transposed.  The others are dropped and counted."""
import itertools

import numpy as np

import canonical_cases as cc
from bensolve_amd import synth
from bensolve_amd.lp import LpEngine, bounds_from_types

T1, T2 = cc.T1, cc.T2
SAME_Y = 1e-9             # y(t1) = y(t2), relative to 1 + |y|
OPT_TOL = 1e-9            # "equals z*", relative to 1 + |z*|
DEGENERATE = 1e-3         # y(-t2), the other end of the optimal face, differs from the canonical y by more


class P1Model:
    """P1(w) of dual_benson (hom = 0), as in tests/test_lp_rev_obj_gpu.py: M = m + q rows, N = n + q columns, variable ids 0..M-1
    rows, M.. columns; rows [A 0; -P I], zero engine cost, the weights w as the cost of the q columns y"""

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


def sparse_covering(m, n, q, seed, per_col=4):
    """covering VLP with a sparse A (per_col non-zeros per column, every row hit) and sparse objectives in which every column of P
    has a non-zero (_sparse_covering of tests/test_lp_rev_obj_gpu.py without its dense columns)"""
    rng = np.random.default_rng(seed)
    prob = synth.covering_vlp(m, n, q, seed)
    A = np.zeros((m, n))
    for j in range(n):
        rows = rng.choice(m, size=per_col, replace=False)
        A[rows, j] = rng.uniform(0.5, 1.5, size=per_col)
    for i in range(m):
        if not A[i].any():
            A[i, rng.integers(n)] = 1.0
    mask = rng.random((q, n)) < 0.3
    mask[rng.integers(q, size=n), np.arange(n)] = True
    P = prob["P"] * mask
    P[:, 0] = prob["P"][:, 0]
    return dict(prob, A=A, P=P)


def decoy_vertices(q):
    """v_k = 2 (1 - e_k): the q vertices of the decoy problem's upper image"""
    return 2.0 * (np.ones((q, q)) - np.eye(q))


def decoy_vlp(q):
    """one row sum x >= 1, x >= 0; the columns of P are the v_k, all midpoints of pairs of them and their centroid.  The feasible set
    has a vertex e_j per column, so every decoy column (midpoint, centroid) is the image of a vertex of the feasible set that is NOT a
    vertex of the image: the upper image conv{v_k} + R^q_+ has exactly the vertices v_k."""
    V = decoy_vertices(q)
    cols = [v for v in V] + [0.5 * (V[i] + V[j]) for i, j in itertools.combinations(range(q), 2)] + [V.mean(axis=0)]
    P = np.array(cols).T
    n = P.shape[1]
    return dict(m=1, n=n, q=q, A=np.ones((1, n)), P=P, optdir=1, rtype=np.full(1, ord("l"), np.uint8), rlb=np.ones(1), rub=np.zeros(1),
                ctype=np.full(n, ord("l"), np.uint8), clb=np.zeros(n), cub=np.zeros(n))


def decoy_weights(q):
    """(1..1) / q, the small-integer vectors with one or two entries doubled, and the vectors with one zero entry, normalised"""
    W = [np.ones(q)]
    for k in (1, 2):
        for idx in itertools.combinations(range(q), k):
            w = np.ones(q); w[list(idx)] = 2.0
            W.append(w)
    for k in range(q):
        w = np.ones(q); w[k] = 0.0
        W.append(w)
    W = np.array(W)
    return W / W.sum(axis=1, keepdims=True)


def covering_weights(prob):
    """the distinct facet normals of the upper image (the expected canonical w of canonical_cases' points on vertices and edges), the
    midpoints of the first 12 pairs of them -- normal to nothing but a vertex's cone, or to an edge -- and six generic weights"""
    q = prob["q"]
    c = cc.build_cases(prob, cc.covering_candidates(prob, 27, 10))
    N = np.unique(np.round(c["w"], 12), axis=0)
    pairs = list(itertools.combinations(range(len(N)), 2))[:12]
    mid = np.array([0.5 * (N[i] + N[j]) for i, j in pairs])
    G = np.random.default_rng(5).uniform(0.2, 1.0, size=(6, q))
    G /= G.sum(axis=1, keepdims=True)
    return np.vstack([N, mid, G]), len(N)


class Highs:
    """P1(w) of one problem for scipy's HiGHS"""

    def __init__(self, prob):
        from scipy.optimize import linprog
        self.linprog = linprog
        self.A, self.P, self.b = np.asarray(prob["A"], float), np.asarray(prob["P"], float), np.asarray(prob["rlb"], float)
        assert all(chr(t) == "l" for t in prob["rtype"]) and all(chr(t) == "l" for t in prob["ctype"]) and not np.any(prob["clb"])

    def p1(self, w):
        """(optimal value, y = P x) of min w.P x, A x >= b, x >= 0"""
        res = self.linprog(self.P.T @ w, A_ub=-self.A, b_ub=-self.b, bounds=[(0.0, None)] * self.A.shape[1], method="highs")
        assert res.status == 0, res.message
        return res.fun, self.P @ res.x


def build_cases(prob, W, facet_normals=0):
    """dict(W, y, z, degenerate, candidates, dropped, facet_normals): the kept weights of W with their expected canonical y"""
    H = Highs(prob)
    d = cc.direction(prob["q"])
    Wk, Y, Z, D = [], [], [], []
    for w in W:
        z0, _ = H.p1(w)
        _, y1 = H.p1(w + T1 * d)
        _, y2 = H.p1(w + T2 * d)
        if np.any(np.abs(y1 - y2) > SAME_Y * (1.0 + np.abs(y2))):
            continue
        if abs(w @ y2 - z0) > OPT_TOL * (1.0 + abs(z0)):
            continue
        _, ym = H.p1(w - T2 * d)
        Wk.append(w); Y.append(y2); Z.append(z0); D.append(np.abs(ym - y2).max() > DEGENERATE)
    return dict(W=np.array(Wk), y=np.array(Y), z=np.array(Z), degenerate=np.array(D, bool), candidates=len(W), dropped=len(W) - len(Wk),
                facet_normals=facet_normals)


def _covering(prob):
    W, nf = covering_weights(prob)
    return prob, W, nf


PROBLEMS = {
    "covering-40x20x4": lambda: _covering(synth.covering_vlp(40, 20, 4, 9)),
    # P1 has 83 columns here: a tableau row crosses 64 columns and one step of the row length (ld = 96)
    "covering-30x80x3": lambda: _covering(synth.covering_vlp(30, 80, 3, 4)),
    # 1603 columns: from 1536 on a selection runs in workgroups of 1024 threads
    "wide-40x1600x3": lambda: _covering(sparse_covering(40, 1600, 3, 7)),
    "decoy-3": lambda: (decoy_vlp(3), decoy_weights(3), 0),
    "decoy-4": lambda: (decoy_vlp(4), decoy_weights(4), 0),
}
COVERING = ("covering-40x20x4", "covering-30x80x3", "wide-40x1600x3")
DECOYS = ("decoy-3", "decoy-4")
_cache = {}


def cases(name):
    """(prob, cases) of a problem, computed once per process and never changed"""
    if name not in _cache:
        prob, W, nf = PROBLEMS[name]()
        c = build_cases(prob, W, nf)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (prob, c)
    return _cache[name]


def check_case_set(c):
    """the conditions a covering case set has to meet before anything is compared against it"""
    kept = len(c["W"])
    assert kept >= 12, "only %d cases kept" % kept
    assert 2 * int(c["degenerate"].sum()) >= kept, "%d of %d kept cases are degenerate" % (int(c["degenerate"].sum()), kept)
    assert 4 * c["dropped"] <= c["candidates"], "%d of %d candidates dropped by the keep rule" % (c["dropped"], c["candidates"])
