"""Bases for bslv_lpq_load_basis (tests/test_lp_basis_gpu.py) and the host's own solution of a basis system.  No GPU in here.

The model is GLPK's, as everywhere: r = A x, variables 0..M-1 auxiliary (rows), M..M+N-1 structural; with K = [I | -A] every point has
K (r, x) = 0, a basis is a set B of M variables with K_B regular, the nonbasic variables rest on the bound their status names and
  basic values     K_B z_B = -K_N z_N
  multipliers      K_B' y = c_B            (c: 0 on the rows, the costs on the columns)
  reduced costs    d_k = c_k - K_k' y      (0 for a basic variable),  objective = c0 + c . x
solve_basis does that by Gaussian elimination with partial pivoting in the precision it is asked for (float64 or np.longdouble).
bases(...) draws, seeded, one basis per structural basic count that sits on an edge of the engine's replay -- 0, 1, KP - 1, KP, KP + 1,
2 KP + 1 and M with KP = 6 pending pivots per pass -- from random column and row sets, and keeps a draw only if the float64 and the
longdouble solution agree to 1e-11 relative: ill-conditioned bases stay out, so a tolerance of 1e-9 tests the engine and not the case.
own_model(...) restates the presolve of bslv_lpq_create (a row with a single non-zero outside the per-LP range becomes a bound of its
column), so that a model with folded rows can be solved on the host in the engine's own indices."""
import numpy as np

BASIC, LOWER, UPPER, FREE, FIXED = 1, 2, 3, 4, 5      # GLPK's GLP_BS .. GLP_NS (include/bslv_hip.h: BSLV_LP_VS_*)
KP = 6
AGREE = 1e-11
LD = np.longdouble


def small_model():
    """a 3 x 5 model with every bound type: (A, lo, up, cost)"""
    A = np.array([[1.0, 2.0, 0.0, -1.0, 0.5], [0.0, 1.0, 1.0, 1.0, 0.0], [2.0, 0.0, -1.0, 0.0, 1.0]])
    inf = np.inf
    lo = np.array([-inf, 1.0, 0.0, 0.0, -2.0, -inf, 1.0, 0.0])
    up = np.array([4.0, 1.0, 6.0, inf, 3.0, inf, 1.0, 5.0])
    cost = np.array([0.5, 1.0, 2.0, 0.0, -1.0, 3.0])
    return A, lo, up, cost


def shape_model(M, N):
    """(A, lo, up, cost) of a shape: lp_cases.random_lp's feasible and bounded LP.  (lp_cases.general_model has two rows with equal
    coefficients: no basis of it has every auxiliary variable nonbasic, and that count is one of the replay's edges.)"""
    import lp_cases as lc
    return lc.random_lp(M, N, np.random.default_rng(500 + M + N), "feasible", bounded=True)


def folded_model():
    """a 9 x 6 random_lp of lp_cases with two rows of a single non-zero: the presolve folds them"""
    import lp_cases as lc
    return lc.random_lp(9, 6, np.random.default_rng(1), "feasible", bounded=True)


def own_model(A, lo, up, first, cnt):
    """(A, lo, up, first, own_of_given) of the engine's own model: bslv_lpq_create's presolve restated"""
    M, N = A.shape
    clo, cup = lo[M:].copy(), up[M:].copy()
    keep = []
    for i in range(M):
        per_lp = cnt > 0 and first <= i < first + cnt
        fold = False
        if not per_lp and M - (i - len(keep)) > 1:
            nz = np.nonzero(A[i])[0]
            if len(nz) == 1 and not (cnt > 0 and first <= M + nz[0] < first + cnt):
                j, a = nz[0], A[i, nz[0]]
                l, u = max(clo[j], lo[i] / a if a > 0 else up[i] / a), min(cup[j], up[i] / a if a > 0 else lo[i] / a)
                if l <= u:
                    fold, clo[j], cup[j] = True, l, u
        if not fold:
            keep.append(i)
    row_in = np.full(M, -1, np.int32)
    row_in[keep] = np.arange(len(keep))
    Mi = len(keep)
    f2 = first if cnt == 0 else (row_in[first] if first < M else Mi + first - M)
    return (A[keep], np.concatenate([lo[keep], clo]), np.concatenate([up[keep], cup]), int(f2),
            np.concatenate([row_in, Mi + np.arange(N, dtype=np.int32)]))


def nonbasic_codes(lo, up, rng):
    """a status for every variable as if it were nonbasic: the bound it has, either of two, FIXED where they are equal, FREE without one"""
    flo, fup = np.isfinite(lo), np.isfinite(up)
    side = rng.random(len(lo)) < 0.5
    return np.where(flo & fup, np.where(lo == up, FIXED, np.where(side, LOWER, UPPER)), np.where(flo, LOWER, np.where(fup, UPPER, FREE))).astype(np.int32)


def nonbasic_values(vstat, lo, up):
    with np.errstate(invalid="ignore"):
        return np.where(vstat == UPPER, up, np.where((vstat == LOWER) | (vstat == FIXED), lo, 0.0))


def _solve(Mat, rhs):
    """Gaussian elimination with partial pivoting in the dtype of Mat; None for a zero pivot"""
    a = np.concatenate([Mat, rhs.reshape(len(Mat), -1)], axis=1).copy()
    n = len(Mat)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if a[p, k] == 0:
            return None
        if p != k:
            a[[k, p]] = a[[p, k]]
        a[k + 1:] -= np.outer(a[k + 1:, k] / a[k, k], a[k])
    x = np.zeros((n, a.shape[1] - n), a.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (a[k, n:] - a[k, k + 1:n] @ x[k + 1:]) / a[k, k]
    return x


def solve_basis(A, lo, up, cost, vstat, dtype=LD):
    """(primal, dual, objective) of the basis vstat over the M + N variables, or None for a singular basis"""
    M, N = A.shape
    K = np.concatenate([np.eye(M), -A], axis=1).astype(dtype)
    c = np.concatenate([np.zeros(M), cost[1:]]).astype(dtype)
    bas = np.nonzero(vstat == BASIC)[0]
    non = np.nonzero(vstat != BASIC)[0]
    assert len(bas) == M
    z = nonbasic_values(vstat, lo, up).astype(dtype)
    z[bas] = 0
    zb = _solve(K[:, bas], -(K[:, non] @ z[non]))
    y = _solve(K[:, bas].T.copy(), c[bas])
    if zb is None or y is None:
        return None
    z[bas] = zb[:, 0]
    d = c - K.T @ y[:, 0]
    d[bas] = 0
    return z, d, dtype(cost[0]) + c[M:] @ z[M:]


def _agree(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(b))))


def well_conditioned(A, lo, up, cost, vstat):
    s64, sld = solve_basis(A, lo, up, cost, vstat, np.float64), solve_basis(A, lo, up, cost, vstat, LD)
    if s64 is None or sld is None:
        return None
    if max(_agree(s64[0], sld[0]), _agree(s64[1], sld[1]), _agree([s64[2]], [sld[2]])) > AGREE:
        return None
    return sld


def counts(M, N):
    """the structural basic counts on the replay's edges that the shape has room for"""
    return sorted({c for c in (0, 1, KP - 1, KP, KP + 1, 2 * KP + 1, M) if c <= min(M, N)})


_BASES = {}


def bases(key, A, lo, up, cost, seed):
    """[(structural basic count, vstat, (primal, dual, objective) in longdouble)], one per count of counts(M, N); computed once per key"""
    if key in _BASES:
        return _BASES[key]
    M, N = A.shape
    rng = np.random.default_rng(seed)
    out = []
    for ns in counts(M, N):
        for attempt in range(400):
            cols = rng.choice(N, size=ns, replace=False)
            rows = rng.choice(M, size=ns, replace=False)
            vstat = nonbasic_codes(lo, up, rng)
            vstat[:M] = np.where(np.isin(np.arange(M), rows), vstat[:M], BASIC)
            vstat[M + cols] = BASIC
            ref = well_conditioned(A, lo, up, cost, vstat)
            if ref is not None:
                out.append((ns, vstat, ref))
                break
        else:
            raise AssertionError("no well-conditioned basis with %d structural basics for %s" % (ns, key))
    _BASES[key] = out
    return out


def singular_basis(A, lo, up, rng_seed=0):
    """(model A with two equal columns, vstat that makes both basic): the basis matrix has two equal columns"""
    M, N = A.shape
    A2 = A.copy()
    A2[:, 1] = A2[:, 0]
    rows = [int(i) for i in np.nonzero(A2[:, 0])[0][:2]]
    if len(rows) < 2:
        rows = [0, 1]
    rng = np.random.default_rng(rng_seed)
    vstat = nonbasic_codes(lo, up, rng)
    vstat[:M] = np.where(np.isin(np.arange(M), rows), vstat[:M], BASIC)
    vstat[M] = vstat[M + 1] = BASIC
    return A2, vstat
