"""Cases for the canonical points of objective batches PER CALL (tests/test_lp_rev_canonical_obj_gpu.py): the five sets of
canonical_obj_cases.PROBLEMS and two WIDE ones for the revised form's tie kernel, k_select_tie_obj_rev -- nothing here touches the GPU.

P1 of sparse_covering(40, n, 3, 11) has N = n + 3 columns.  n = 2045: N = 2048, one slice of a tableau row, "(ld + 2047) / 2048" is 1 and
the LP's own workgroup does all the sparse products.  n = 2046: N = 2049, ld goes on to the next step, the quotient is 2: the first
shape with a helper workgroup beside the LP's own.  Weights, expected canonical y (HiGHS on the shifted weights) and the keep rule are
canonical_obj_cases' (covering_weights / build_cases / check_case_set); seed 11 meets check_case_set at both sizes (seed 7, the one of
wide-40x1600x3, fails the degenerate share at n = 2046).  Each set takes about 9 s of HiGHS, once per process."""
import canonical_obj_cases as co

from bensolve_amd import synth

WIDE = {2048: "wide-40x2045x3", 2049: "wide-40x2046x3"}      # columns of P1 -> name
# the problems alone (a child process that is handed the weights needs no HiGHS)
VLP = {
    "covering-40x20x4": lambda: synth.covering_vlp(40, 20, 4, 9),
    "covering-30x80x3": lambda: synth.covering_vlp(30, 80, 3, 4),
    "wide-40x1600x3": lambda: co.sparse_covering(40, 1600, 3, 7),
    "decoy-3": lambda: co.decoy_vlp(3),
    "decoy-4": lambda: co.decoy_vlp(4),
    "wide-40x2045x3": lambda: co.sparse_covering(40, 2045, 3, 11),
    "wide-40x2046x3": lambda: co.sparse_covering(40, 2046, 3, 11),
}
PROBLEMS = dict(co.PROBLEMS)
PROBLEMS["wide-40x2045x3"] = lambda: co._covering(VLP["wide-40x2045x3"]())
PROBLEMS["wide-40x2046x3"] = lambda: co._covering(VLP["wide-40x2046x3"]())
COVERING = co.COVERING + tuple(WIDE.values())
DECOYS = co.DECOYS
ALL = COVERING + DECOYS
_cache = {}


def cases(name):
    """(prob, cases) of a problem, computed once per process and never changed; the five sets of canonical_obj_cases are its own"""
    if name in co.PROBLEMS:
        return co.cases(name)
    if name not in _cache:
        prob, W, nf = PROBLEMS[name]()
        c = co.build_cases(prob, W, nf)
        for a in c.values():
            if hasattr(a, "setflags"):
                a.setflags(write=False)
        _cache[name] = (prob, c)
    return _cache[name]
