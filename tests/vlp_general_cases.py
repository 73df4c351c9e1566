"""CPU: small GENERAL vector linear programs for the solution-file tests (tests/test_solution_cases.py, tests/test_solutions_gpu.py):
rows of every type, singleton rows that the driver's presolve folds into column bounds, boxed and half-bounded columns, min and
max, bounded and unbounded upper images, ordering cones given by generators of the cone or of its dual.

Deterministic from synth.splitmix64_stream (no np.random: tests/golden/solutions.* belong to bit-identical inputs on every machine);
coefficients are rounded to three decimals.  CASES maps a name to a builder; BOUNDED names the cases that also run with -b."""
import hashlib

import numpy as np

from bensolve_amd import synth


class _Stream:
    def __init__(self, seed, count=4096):
        self.u, self.k = synth.splitmix64_stream(seed, count), 0

    def take(self, shape, lo=0.0, hi=1.0):
        n = int(np.prod(shape))
        out = self.u[self.k:self.k + n].reshape(shape)
        assert out.size == n
        self.k += n
        return lo + (hi - lo) * out


def bounded_general(m, n, q, seed, optdir=1):
    """Interior point x0, A about 70 % dense with mixed signs; the first max(2, n // 3) rows are singletons (coefficients 2, -1, 0.5,
    types d, l, u), the others cycle d, l, u, d and the last row is 's'; every row bound lies 0.3 to 1.0 away from A x0 (the 's' row
    passes through x0); all columns 'd' around x0, so the feasible set is bounded; P uniform in [-1, 1]."""
    s = _Stream(seed)
    A = np.round(s.take((m, n), -1, 1), 3) * (s.take((m, n)) < 0.7)
    x0 = np.round(s.take(n, 0.5, 1.5), 3)
    ns = max(2, n // 3)
    for i in range(ns):
        A[i] = 0.0
        A[i, i] = (2.0, -1.0, 0.5)[i % 3]
    r = A @ x0
    w = s.take(m, 0.3, 1.0)
    rtype = np.empty(m, np.uint8); rlb = np.zeros(m); rub = np.zeros(m)
    for i in range(m):
        t = "dlu"[i % 3] if i < ns else "dlud"[(i - ns) % 4]
        if i == m - 1:
            t = "s"
        rtype[i] = ord(t)
        rlb[i] = np.round(r[i] - w[i], 3) if t in "ld" else (np.round(r[i], 3) if t == "s" else 0.0)
        rub[i] = np.round(r[i] + w[i], 3) if t in "ud" else 0.0
    # (the rounded 's' bound passes within 5e-4 of A x0, every other bound is at least 0.3 away: the feasible set keeps an interior
    # point of that hyperplane)
    P = np.round(s.take((q, n), -1, 1), 3)
    return dict(m=m, n=n, q=q, A=A, P=P, optdir=optdir, rtype=rtype, rlb=rlb, rub=rub,
                ctype=np.full(n, ord("d"), np.uint8), clb=np.round(x0 - 1.0, 3), cub=np.round(x0 + 1.0, 3))


def unbounded_general(m, n, q, seed, optdir=1):
    """The first n // 2 columns are 'd', the rest 'l' (unbounded above) with A >= 0 on them; rows 0 and 1 are singleton 'l' rows on
    unbounded columns; every third row has mixed signs on the boxed columns only and type 'd' or 'u', the rest are 'l'.  P uniform in
    [-1, 1] except its last row = column sums of |P| over the other rows + 0.1 .. 0.5: the sum of the objectives has positive
    coefficients, so it is bounded below on the feasible set and the upper image has a vertex.  optdir = -1 negates P."""
    s = _Stream(seed)
    nb = n // 2
    A = np.round(s.take((m, n)), 3) * (s.take((m, n)) < 0.7)
    mixed = np.round(s.take((m, nb), -1, 1), 3)
    x0 = np.round(s.take(n, 0.5, 1.5), 3)
    w = s.take(m, 0.3, 1.0)
    rtype = np.empty(m, np.uint8); rlb = np.zeros(m); rub = np.zeros(m)
    for i in range(m):
        if i < 2:
            A[i] = 0.0
            A[i, nb + i] = (2.0, 0.5)[i]
            t = "l"
        elif i % 3 == 0:
            A[i, nb:] = 0.0
            A[i, :nb] = mixed[i]
            t = "du"[i % 2]
        else:
            t = "l"
        r = A[i] @ x0
        rtype[i] = ord(t)
        rlb[i] = np.round(r - w[i], 3) if t in "ld" else 0.0
        rub[i] = np.round(r + w[i], 3) if t in "ud" else 0.0
    ctype = np.array([ord("d")] * nb + [ord("l")] * (n - nb), np.uint8)
    P = np.round(s.take((q, n), -1, 1), 3)
    P[q - 1] = np.round(np.abs(P[:q - 1]).sum(axis=0) + s.take(n, 0.1, 0.5), 3)
    if optdir == -1:
        P = -P
    return dict(m=m, n=n, q=q, A=A, P=P, optdir=optdir, rtype=rtype, rlb=rlb, rub=rub,
                ctype=ctype, clb=np.round(x0 - 1.0, 3), cub=np.where(ctype == ord("d"), np.round(x0 + 1.0, 3), 0.0))


def with_cone(prob, kind, gen, c=None):
    """kind "cone": gen (q x k, generators as columns) spans the ordering cone C; "dualcone": it spans C+.  c: the duality parameter."""
    out = dict(prob)
    out.update(cone_kind={"cone": 1, "dualcone": 2}[kind], gen=np.array(gen, np.float64).reshape(prob["q"], -1),
               c=None if c is None else np.array(c, np.float64))
    return out


def boxed_lattice(m, n, q, seed):
    """synth.degenerate_vlp at a small size: every column is free and boxed by a singleton 'd 0 1' row, so every column bound the LP
    engine sees comes from a folded row."""
    return synth.degenerate_vlp(m, n, q, seed)


_E3 = np.eye(3)
CASES = {
    "B3": lambda: bounded_general(14, 9, 3, 1, 1),
    "B3max": lambda: bounded_general(14, 9, 3, 2, -1),
    "B3max-cone": lambda: with_cone(bounded_general(14, 9, 3, 2, -1), "cone", np.column_stack([_E3, [1, 1, -0.5]]), [1, 1, 2]),
    "U2": lambda: unbounded_general(12, 8, 2, 1, 1),
    "U2-dualcone": lambda: with_cone(unbounded_general(12, 8, 2, 1, 1), "dualcone", np.array([[2.0, 1.0], [1.0, 2.0]])),
    "U3": lambda: unbounded_general(14, 9, 3, 2, 1),
    "U3max": lambda: unbounded_general(14, 9, 3, 19, -1),
    "U3-cone": lambda: with_cone(unbounded_general(14, 9, 3, 2, 1), "cone", np.column_stack([_E3, [1, 1, -0.5], [1, -0.25, 1]]), [1, 2, 1]),
    "U4": lambda: unbounded_general(14, 8, 4, 6, 1),
    "L3": lambda: boxed_lattice(14, 6, 3, 13),
}
BOUNDED = ("B3", "B3max", "B3max-cone", "L3")


def singleton_rows(prob):
    return np.flatnonzero(np.count_nonzero(prob["A"], axis=1) == 1)


def digest(prob):
    """SHA-256 of the input arrays (little-endian float64 / uint8, fixed order), the sizes, the sense and the cone data"""
    h = hashlib.sha256()
    h.update(np.array([prob["m"], prob["n"], prob["q"], prob["optdir"], int(prob.get("cone_kind") or 0)], "<i8").tobytes())
    for k in ("A", "P", "rlb", "rub", "clb", "cub"):
        h.update(np.ascontiguousarray(prob[k], "<f8").tobytes())
    for k in ("rtype", "ctype"):
        h.update(np.ascontiguousarray(prob[k], np.uint8).tobytes())
    for k in ("gen", "c"):
        if prob.get(k) is not None:
            h.update(np.ascontiguousarray(prob[k], "<f8").tobytes())
    return h.hexdigest()
