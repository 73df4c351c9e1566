"""Cases for the canonical-dual tests (tests/test_lp_canonical_gpu.py, tests/test_benson_canonical_gpu.py): problems, points v
whose ray v + z c meets faces of lower dimension of the upper image, and the EXPECTED canonical dual w of P2(v) from scipy's HiGHS --
nothing here touches the GPU or oracle/.

The canonical dual of P2(v) for a direction d is the dual P2(v + t d) has for all small t > 0 (include/bslv_hip.h,
bslv_lpq_set_canonical).  HiGHS knows no such rule, but it can solve the shifted LPs: the value function of P2 is convex and piecewise
linear in t, so a w that is the dual at t1 = 2^-10 AND at t2 = 2^-11 and is still optimal at t = 0 is the slope of one linear piece
that reaches from 0 to t1 -- the unique optimal dual on (0, t2].  A case is KEPT only if both hold (keep rule); the others are dropped
and counted.

P2(v) as written down here, from the problem data alone (rows 'l', columns 'l' or 'f', c = (1..1), default cone R = I):
    min z   s.t.  A x >= b (u >= 0),   P x - z c <= v (w >= 0),   x >= 0 or free
and its dual    max b.u - v.w   s.t.  A'u - P'w <= 0 (= 0 for a free column),  c.w = 1,  u, w >= 0."""
import numpy as np

T1, T2 = 2.0 ** -10, 2.0 ** -11
SAME_W = 1e-12            # w(t1) = w(t2)
OPT_TOL = 1e-9            # "equals z*", relative to 1 + |z*|
DEGENERATE = 1e-3         # spread of some w_k over the optimal face at t = 0


def hash01(k):
    """the engine's hash01 (bensolve_amd/csrc/common.h)"""
    x = (k * 2654435761) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    return (x >> 8) / 16777216.0


def direction(q):
    """d_k = 1 + hash01(k): the driver's fixed generic direction (bslv_benson_set_canonical); with R = I also dir_j of the LP engine"""
    return np.array([1.0 + hash01(k) for k in range(q)])


def octahedron_vlp():
    """P = I on the octahedron |x|_1 <= 1 (eight rows sum +-x_i >= -1, x free): the upper image is
    {y : sum_{i in S} y_i >= -1 for every non-empty S of {1,2,3}} -- seven facets"""
    A = np.array([[s0, s1, s2] for s0 in (1.0, -1.0) for s1 in (1.0, -1.0) for s2 in (1.0, -1.0)])
    return dict(m=8, n=3, q=3, A=A, P=np.eye(3), optdir=1, rtype=np.full(8, ord("l"), np.uint8), rlb=-np.ones(8), rub=np.zeros(8),
                ctype=np.full(3, ord("f"), np.uint8), clb=np.zeros(3), cub=np.zeros(3))


def octahedron_normals():
    """the seven facet normals scaled to c.w = 1"""
    out = []
    for mask in range(1, 8):
        s = np.array([(mask >> k) & 1 for k in range(3)], float)
        out.append(s / s.sum())
    return np.array(out)


def hypercube_vlp(q=4):
    """P = I on [0,1]^q (rows x_i <= 1 written as -x_i >= -1, x >= 0): the upper image is the orthant at the origin, q facets"""
    return dict(m=q, n=q, q=q, A=-np.eye(q), P=np.eye(q), optdir=1, rtype=np.full(q, ord("l"), np.uint8), rlb=-np.ones(q), rub=np.zeros(q),
                ctype=np.full(q, ord("l"), np.uint8), clb=np.zeros(q), cub=np.zeros(q))


class Highs:
    """P2(v) of one problem and the LPs around it, for scipy's HiGHS"""

    def __init__(self, prob):
        from scipy.optimize import linprog
        self.linprog = linprog
        A, P = np.asarray(prob["A"], float), np.asarray(prob["P"], float)
        self.m, self.n = A.shape
        self.q = P.shape[0]
        assert all(chr(t) == "l" for t in prob["rtype"]) and all(chr(t) in "lf" for t in prob["ctype"]) and not np.any(prob["clb"])
        self.A, self.P, self.b = A, P, np.asarray(prob["rlb"], float)
        self.free = np.array([chr(t) == "f" for t in prob["ctype"]])
        self.xb = [(None, None) if f else (0.0, None) for f in self.free]
        self.Aub = np.vstack([np.hstack([-A, np.zeros((self.m, 1))]), np.hstack([P, -np.ones((self.q, 1))])])
        self.cost = np.concatenate([np.zeros(self.n), [1.0]])

    def p2(self, v):
        """(z*, w, y) of P2(v)"""
        res = self.linprog(self.cost, A_ub=self.Aub, b_ub=np.concatenate([-self.b, v]), bounds=self.xb + [(None, None)], method="highs")
        assert res.status == 0, res.message
        return res.fun, -res.ineqlin.marginals[self.m:], self.P @ res.x[:self.n]

    def value_at(self, w, v):
        """the dual objective at w, maximised over u: min over x in S of w.(P x - v)"""
        res = self.linprog(self.P.T @ w, A_ub=-self.A, b_ub=-self.b, bounds=self.xb, method="highs")
        assert res.status == 0, res.message
        return res.fun - w @ v

    def dual_spread(self, v, zstar):
        """largest max - min of a w_k over the optimal dual face of P2(v)"""
        m, q = self.m, self.q
        G = np.hstack([self.A.T, -self.P.T])                     # A'u - P'w
        face = np.concatenate([-self.b, v])[None, :]             # -(b.u - v.w) <= -z* + tol
        Aub = np.vstack([G[~self.free], face])
        bub = np.concatenate([np.zeros(int((~self.free).sum())), [-zstar + OPT_TOL * (1.0 + abs(zstar))]])
        Aeq = np.vstack([G[self.free], np.concatenate([np.zeros(m), np.ones(q)])[None, :]])
        beq = np.concatenate([np.zeros(int(self.free.sum())), [1.0]])
        spread = 0.0
        for k in range(q):
            e = np.zeros(m + q); e[m + k] = 1.0
            lo = self.linprog(e, A_ub=Aub, b_ub=bub, A_eq=Aeq, b_eq=beq, bounds=[(0.0, None)] * (m + q), method="highs")
            hi = self.linprog(-e, A_ub=Aub, b_ub=bub, A_eq=Aeq, b_eq=beq, bounds=[(0.0, None)] * (m + q), method="highs")
            assert lo.status == 0 and hi.status == 0, (lo.message, hi.message)
            spread = max(spread, -hi.fun - lo.fun)
        return spread

    def vertex(self, lam):
        """a vertex of the upper image: P x of a minimiser of the weighted sum lam.P x over S"""
        res = self.linprog(self.P.T @ lam, A_ub=-self.A, b_ub=-self.b, bounds=self.xb, method="highs")
        assert res.status == 0, res.message
        return self.P @ res.x


def build_cases(prob, candidates):
    """dict(V, w, z, degenerate, candidates, dropped): the kept cases of `candidates` with their expected canonical w"""
    H = Highs(prob)
    d = direction(H.q)
    V, W, Z, D = [], [], [], []
    for v in candidates:
        z0, _, _ = H.p2(v)
        _, w1, _ = H.p2(v + T1 * d)
        _, w2, _ = H.p2(v + T2 * d)
        if np.abs(w1 - w2).max() > SAME_W:
            continue
        if abs(H.value_at(w2, v) - z0) > OPT_TOL * (1.0 + abs(z0)):
            continue
        V.append(v); W.append(w2); Z.append(z0); D.append(H.dual_spread(v, z0) > DEGENERATE)
    return dict(V=np.array(V), w=np.array(W), z=np.array(Z), degenerate=np.array(D, bool), candidates=len(candidates), dropped=len(candidates) - len(V))


def octahedron_candidates():
    """points of the lattice (Z/2)^3 below the image (every coordinate <= -1, so y_1 + y_2 + y_3 >= -1 is violated).  Where the ray
    meets the image is known in closed form -- z = max over S of (-1 - sum_S v) / |S| -- and so is the number of facets through that
    point: the candidates are the lattice points whose ray meets an edge or a vertex (two facets or more) and, for the unique case,
    the first eight that meet a facet in its interior."""
    g = (-3.0, -2.5, -2.0, -1.5, -1.0)
    N = octahedron_normals()
    low, facet = [], []
    for a in g:
        for b in g:
            for c in g:
                v = np.array([a, b, c])
                size = (N > 0).sum(axis=1)
                zs = (-1.0 / size) - N @ v                   # (-1 - sum_S v) / |S|
                tight = int((zs >= zs.max() - 1e-12).sum())
                (low if tight >= 2 else facet).append(v)
    return low + facet[:8]


def covering_candidates(prob, nweights, npairs):
    """Covering problems have real data: no lattice of R^q meets their edges.  The points are v = y - c for y a vertex of the image
    (minimisers of weighted sums with small integer weights: the ray from v meets the image in the vertex itself) and for y the
    midpoint of two of those vertices (an edge of the image where the two are adjacent, a face of higher dimension or a point above
    the boundary where they are not)."""
    H = Highs(prob)
    q = H.q
    Y = []
    lam = np.ones(q)
    for k in range(nweights):                       # 1..3 per objective, counted through in base 3
        lam = np.array([1.0 + (k // 3 ** i) % 3 for i in range(q)])
        y = H.vertex(lam)
        if not any(np.abs(y - y0).max() < 1e-9 for y0 in Y):
            Y.append(y)
    out = [y - 1.0 for y in Y]
    pairs = [(i, j) for i in range(len(Y)) for j in range(i + 1, len(Y))]
    for i, j in pairs[:npairs]:
        out.append(0.5 * (Y[i] + Y[j]) - 1.0)
    return out


def _covering(m, n, q, seed, nweights, npairs):
    from bensolve_amd import synth
    prob = synth.covering_vlp(m, n, q, seed)
    return prob, covering_candidates(prob, nweights, npairs)


PROBLEMS = {
    "octahedron": lambda: (octahedron_vlp(), octahedron_candidates()),
    "covering-40x20x4": lambda: _covering(40, 20, 4, 9, 27, 10),
    # P2 has 84 columns here: a tableau row crosses 64 columns and one step of the row length (ld = 96)
    "covering-30x80x3": lambda: _covering(30, 80, 3, 4, 27, 10),
}
# Wide sets: P2 of covering_vlp(24, n, q, seed) has N = n + q + 1 columns, one on each side of a threshold of the launch code
# (tests/test_lp_canonical_gpu.py names them).  q = 3: M + 1 = 32 rows, the last row tile of a pass is full; q = 4: 34, it holds one row.
# N -> (n, q, seed, nweights, npairs), chosen on the CPU (python tests/canonical_cases.py prints what each set keeps).  The sets
# with q = 4 take 18 weights and 3 pairs: with 27 and 10 (34 and 37 candidates, 28 and 34 kept) they need 11 s and 15 s to build.
WIDE = {256: (252, 3, 1, 27, 10), 257: (253, 3, 1, 27, 10), 1120: (1116, 3, 2, 27, 10), 1121: (1117, 3, 2, 27, 10),
        1535: (1531, 3, 3, 27, 10), 1536: (1532, 3, 3, 27, 10), 2048: (2043, 4, 4, 18, 3), 2049: (2044, 4, 4, 18, 3)}
WIDE_NAMES = {N: "wide-24x%dx%d" % v[:2] for N, v in WIDE.items()}
for _N, _v in WIDE.items():
    PROBLEMS[WIDE_NAMES[_N]] = lambda v=_v: _covering(24, v[0], v[1], v[2], v[3], v[4])
_cache = {}


def cases(name):
    """(prob, cases) of a problem, computed once per process and never changed"""
    if name not in _cache:
        prob, cand = PROBLEMS[name]()
        c = build_cases(prob, cand)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (prob, c)
    return _cache[name]


def check_case_set(c):
    """the conditions a case set has to meet before anything is compared against it"""
    kept = len(c["V"])
    assert kept >= 12, "only %d cases kept" % kept
    assert 2 * int(c["degenerate"].sum()) >= kept, "%d of %d kept cases are degenerate" % (int(c["degenerate"].sum()), kept)
    assert 4 * c["dropped"] <= c["candidates"], "%d of %d candidates dropped by the keep rule" % (c["dropped"], c["candidates"])


if __name__ == "__main__":
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in sys.argv[1:] or sorted(PROBLEMS):
        t0 = time.time()
        prob, c = cases(name)
        check_case_set(c)
        print("canonical_cases %s: m %d n %d q %d candidates %d kept %d degenerate %d dropped %d (%.1f s)" % (
            name, prob["m"], prob["n"], prob["q"], c["candidates"], len(c["V"]), int(c["degenerate"].sum()), c["dropped"], time.time() - t0), flush=True)
