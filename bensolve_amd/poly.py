"""Host-side mirror of the reference's polyhedron interface (bslv_poly.h:90-118) over the HIP engine."""
import ctypes
import numpy as np
from ._lib import load_library, check

CONE_POLAR, LOWER2UPPER, UPPER2LOWER = 0, 1, 2
_bound = False


def _bind(lib):
    global _bound
    if _bound:
        return
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.bslv_poly_create.argtypes = [ctypes.POINTER(vp), i, i, vp]
    lib.bslv_poly_destroy.argtypes = [vp]
    lib.bslv_poly_destroy.restype = None
    lib.bslv_poly_dual0_apex.argtypes = [vp]
    lib.bslv_poly_add.argtypes = [vp, vp, i, vp]
    lib.bslv_poly_add_cuts.argtypes = [vp, i, vp, vp, vp]
    lib.bslv_poly_init.argtypes = [vp, vp]
    lib.bslv_poly_set_batch_mode.argtypes = [vp, i]
    lib.bslv_poly_rounds_run.argtypes = [vp]
    lib.bslv_poly_rounds_run.restype = ctypes.c_long
    lib.bslv_poly_debug_set.argtypes = [vp, ctypes.c_int, ctypes.c_long]
    lib.bslv_poly_debug_set.restype = ctypes.c_int
    lib.bslv_poly_path_stats.argtypes = [vp, vp]
    lib.bslv_poly_path_stats.restype = ctypes.c_int
    lib.bslv_poly_next.argtypes = [vp, vp, vp, vp, vp]
    lib.bslv_poly_unprocessed.argtypes = [vp, i, vp, vp, vp, vp]
    lib.bslv_poly_mark.argtypes = [vp, i, vp]
    lib.bslv_poly_dual_adjacency.argtypes = [vp]
    lib.bslv_poly_classify_batch.argtypes = [vp, i, vp, vp, vp, i, vp]
    if hasattr(lib, "bslv_poly_classify_batch_touch"):                  # (TEST entry; absent from older builds used in A/B probes)
        lib.bslv_poly_classify_batch_touch.argtypes = [vp, i, vp, vp, vp, vp]
    lib.bslv_poly_bench_fill.argtypes = [vp, i, ctypes.c_ulonglong]
    for n in ("dim", "nprimal", "ndual"):
        getattr(lib, "bslv_poly_" + n).argtypes = [vp]
    for n in ("nedges", "ninc", "ndual_edges", "pair_tests", "new_vertices"):
        f = getattr(lib, "bslv_poly_" + n)
        f.argtypes = [vp]
        f.restype = ctypes.c_long
    lib.bslv_poly_get_primal.argtypes = [vp, vp, vp, vp, vp]
    lib.bslv_poly_get_dual.argtypes = [vp, vp, vp, vp]
    lib.bslv_poly_get_edges.argtypes = [vp, vp]
    lib.bslv_poly_get_inc.argtypes = [vp, vp]
    lib.bslv_poly_get_dual_edges.argtypes = [vp, vp]
    _bound = True


class PolyEngine:
    """poly_args-like object: primal polyhedron + dual, living in HBM."""

    def __init__(self, dim, v2h=CONE_POLAR, c=None):
        self.lib = load_library()
        _bind(self.lib)
        self.d = dim
        cc = None if c is None else np.ascontiguousarray(c, np.float64)
        h = ctypes.c_void_p()
        check(self.lib.bslv_poly_create(ctypes.byref(h), dim, v2h, None if cc is None else cc.ctypes.data))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.bslv_poly_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dual0_apex(self):
        check(self.lib.bslv_poly_dual0_apex(self.h))

    def add(self, val, ideal=0):
        """poly__add_vrtx: 0 = added/queued, 1 = redundant"""
        v = np.ascontiguousarray(val, np.float64)
        rc = ctypes.c_int()
        check(self.lib.bslv_poly_add(self.h, v.ctypes.data, int(ideal), ctypes.byref(rc)))
        return rc.value

    def add_cuts(self, vals, ideals=None):
        vals = np.ascontiguousarray(vals, np.float64).reshape(-1, self.d)
        B = len(vals)
        rc = np.zeros(B, np.int32)
        idl = None if ideals is None else np.ascontiguousarray(ideals, np.int32)
        check(self.lib.bslv_poly_add_cuts(self.h, B, vals.ctypes.data, None if idl is None else idl.ctypes.data, rc.ctypes.data))
        return rc

    def set_batch_mode(self, mode):
        check(self.lib.bslv_poly_set_batch_mode(self.h, int(mode)))

    def rounds_run(self):
        return self.lib.bslv_poly_rounds_run(self.h)

    def debug_set(self, key, value):
        check(self.lib.bslv_poly_debug_set(self.h, int(key), int(value)))

    def rounds2_stats(self):
        out = (ctypes.c_long * 5)()
        self.lib.bslv_poly_rounds2_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_rounds2_stats(self.h, out))
        return dict(rounds=out[0], cuts=out[1], chunks=out[2], fallback_prunes=out[3], declined=out[4])

    def split_stats(self):
        """rounds: prunes that were worked in parts by several workgroups of their launch, helper workgroups that took a part"""
        out = (ctypes.c_long * 2)()
        self.lib.bslv_poly_split_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_split_stats(self.h, out))
        return dict(split_prunes=out[0], helper_parts=out[1])

    def rounds2_health(self):
        """(cuts handed back late, mailbox reads repeated because the sequence number arrived before the state)"""
        for f in ("bslv_poly_rounds2_late_left", "bslv_poly_rounds2_torn_reads"):
            getattr(self.lib, f).restype = ctypes.c_long
            getattr(self.lib, f).argtypes = [ctypes.c_void_p]
        return dict(late_left=self.lib.bslv_poly_rounds2_late_left(self.h), torn_reads=self.lib.bslv_poly_rounds2_torn_reads(self.h))

    def sharded_prunes(self):
        """multi-GPU: adjacency prunes whose pair space was dealt to the ranks"""
        self.lib.bslv_poly_sharded_prunes.restype = ctypes.c_long
        self.lib.bslv_poly_sharded_prunes.argtypes = [ctypes.c_void_p]
        return self.lib.bslv_poly_sharded_prunes(self.h)

    def set_prune_window(self, blocks):
        """the most pair blocks (one row, 256 columns) a window of a large facet's adjacency prune may hold; 0 = default"""
        self.lib.bslv_poly_set_prune_window.argtypes = [ctypes.c_void_p, ctypes.c_long]
        check(self.lib.bslv_poly_set_prune_window(self.h, int(blocks)))

    def get_prune_window(self):
        self.lib.bslv_poly_get_prune_window.restype = ctypes.c_long
        self.lib.bslv_poly_get_prune_window.argtypes = [ctypes.c_void_p]
        return self.lib.bslv_poly_get_prune_window(self.h)

    def prune_window_stats(self):
        """(prunes that ran in more than one window, their windows in total, most pair blocks any window held)"""
        out = (ctypes.c_long * 3)()
        self.lib.bslv_poly_prune_window_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_prune_window_stats(self.h, out))
        return list(out)

    @staticmethod
    def selftest_pair_blocks(nm, window_blocks=0, samples=100000):
        """index arithmetic of a windowed prune of a facet of nm members, no polyhedron needed:
        [windows, pair blocks in total, sampled pairs mapped wrongly, largest relative block id]"""
        lib = load_library()
        out = (ctypes.c_long * 4)()
        lib.bslv_selftest_pair_blocks.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
        check(lib.bslv_selftest_pair_blocks(int(nm), int(window_blocks), int(samples), out))
        return list(out)

    def set_snap(self, on=1):
        """the projection sub-band of poly__cut (bslv_poly.c:666-674); cuts are then applied one at a time"""
        self.lib.bslv_poly_set_snap.argtypes = [ctypes.c_void_p, ctypes.c_int]
        check(self.lib.bslv_poly_set_snap(self.h, on))

    def snapped(self):
        out = ctypes.c_long()
        self.lib.bslv_poly_snapped.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_snapped(self.h, ctypes.byref(out)))
        return out.value

    def path_stats(self):
        out = (ctypes.c_long * 6)()
        check(self.lib.bslv_poly_path_stats(self.h, out))
        return dict(hot_chunks=out[0], speculative=out[1], declined=out[2], prune_fallbacks=out[3], single_cuts=out[4], member_list_prunes=out[5])

    def init(self):
        rc = ctypes.c_int()
        check(self.lib.bslv_poly_init(self.h, ctypes.byref(rc)))
        return rc.value

    def next(self):
        v = np.empty(self.d)
        ideal, idx, rc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(self.lib.bslv_poly_next(self.h, v.ctypes.data, ctypes.byref(ideal), ctypes.byref(idx), ctypes.byref(rc)))
        return None if rc.value else (v, ideal.value, idx.value)

    def unprocessed(self, max_out=None):
        cnt = ctypes.c_int()
        check(self.lib.bslv_poly_unprocessed(self.h, 0, None, None, None, ctypes.byref(cnt)))
        n = cnt.value if max_out is None else min(cnt.value, max_out)
        idx = np.empty(n, np.int32)
        val = np.empty((n, self.d))
        ideal = np.empty(n, np.int32)
        if n:
            check(self.lib.bslv_poly_unprocessed(self.h, n, idx.ctypes.data, val.ctypes.data, ideal.ctypes.data, ctypes.byref(cnt)))
        return idx, val, ideal, cnt.value

    def mark(self, idx):
        idx = np.ascontiguousarray(np.atleast_1d(idx), np.int32)
        check(self.lib.bslv_poly_mark(self.h, len(idx), idx.ctypes.data))

    def dual_adjacency(self):
        check(self.lib.bslv_poly_dual_adjacency(self.h))

    def classify_batch(self, hps, repeats=1, fetch=True):
        hps = np.ascontiguousarray(hps, np.float64).reshape(-1, self.d + 1)
        B = len(hps)
        nv = self.lib.bslv_poly_nprimal(self.h)
        words = np.zeros(((B + 31) // 32, nv), np.uint64) if fetch else None
        anym = np.zeros(B, np.int32)
        ms = ctypes.c_float()
        check(self.lib.bslv_poly_classify_batch(self.h, B, hps.ctypes.data, None if words is None else words.ctypes.data,
                                                anym.ctypes.data, repeats, ctypes.byref(ms)))
        return words, anym, ms.value

    def classify_batch_touch(self, hps):
        """TEST: K1 as the chunked cut application launches it -> (words, touch counts, first touched halfspace)"""
        hps = np.ascontiguousarray(hps, np.float64).reshape(-1, self.d + 1)
        B = len(hps)
        nv = self.lib.bslv_poly_nprimal(self.h)
        words = np.zeros(((B + 31) // 32, nv), np.uint64)
        tc, t1 = np.zeros(nv, np.int32), np.zeros(nv, np.int32)
        check(self.lib.bslv_poly_classify_batch_touch(self.h, B, hps.ctypes.data, words.ctypes.data, tc.ctypes.data, t1.ctypes.data))
        return words, tc, t1

    def bench_fill(self, nv, seed=1):
        check(self.lib.bslv_poly_bench_fill(self.h, int(nv), int(seed)))

    CHECK_FIELDS = ("elements", "facets", "incidences", "bad_incidences", "unlisted_incidences", "infeasible",
                    "edges", "bad_edges", "duplicate_edges", "passing_pairs", "missing_edges", "extra_edges")

    def check(self, tol=0, rows=None, max_offenders=64):
        """bslv_poly_check: the consistency check of the resident polyhedron (poly__polyck and its converse).
        rows = (first, count) of the live elements whose pairs are scanned, None = all.  Returns the twelve counts by name and as
        the list `out`, `worst` = (largest residual of a listed incidence, most negative slack), `offenders` = sorted (kind, a, b)
        tuples (at most max_offenders) and their total `n_offenders`; `clean` = every defect count is zero."""
        first, count = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
        out = (ctypes.c_long * 12)()
        worst = (ctypes.c_double * 2)()
        off = np.zeros((max(int(max_offenders), 0), 3), np.int32)
        n_off = ctypes.c_int()
        f = self.lib.bslv_poly_check
        f.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_int, ctypes.c_void_p]
        check(f(self.h, float(tol), first, count, out, worst, off.ctypes.data if len(off) else None, int(max_offenders), ctypes.byref(n_off)))
        res = dict(zip(self.CHECK_FIELDS, out))
        res["out"] = list(out)
        res["worst"] = (worst[0], worst[1])
        res["n_offenders"] = n_off.value
        res["offenders"] = [tuple(int(v) for v in r) for r in off[:min(n_off.value, len(off))]]
        res["clean"] = not any(out[k] for k in (3, 4, 5, 7, 8, 10, 11))
        return res

    GARBAGE_FIELDS = ("slots", "live", "pool_used", "pool_live", "edges", "bytes")
    COMPACT_STAT_FIELDS = ("calls", "slots_removed", "pool_removed", "bytes_returned", "slots_removed_total", "pool_removed_total",
                           "us", "us_total")

    def garbage(self):
        """bslv_poly_garbage: live / garbage figures of the resident polyhedron by name (and as the list `out`); read-only"""
        out = (ctypes.c_long * 6)()
        self.lib.bslv_poly_garbage.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_garbage(self.h, out))
        res = dict(zip(self.GARBAGE_FIELDS, [int(v) for v in out]))
        res["out"] = [int(v) for v in out]
        return res

    def compact(self):
        """bslv_poly_compact: the live elements become 0 .. live-1 in ascending order of their old slots, their lists are packed.
        Returns (new_of_old, figures after the call); new_of_old[i] = -1 for a dead slot.  Element ids taken before are stale."""
        n = self.lib.bslv_poly_nprimal(self.h)
        new_of_old = np.full(n, -1, np.int32)
        out = (ctypes.c_long * 6)()
        self.lib.bslv_poly_compact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_compact(self.h, new_of_old.ctypes.data if n else None, out))
        res = dict(zip(self.GARBAGE_FIELDS, [int(v) for v in out]))
        res["out"] = [int(v) for v in out]
        return new_of_old, res

    def last_compact_stats(self):
        """bslv_poly_last_compact_stats by name (and as the list `out`)"""
        out = (ctypes.c_long * 8)()
        self.lib.bslv_poly_last_compact_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        check(self.lib.bslv_poly_last_compact_stats(self.h, out))
        res = dict(zip(self.COMPACT_STAT_FIELDS, [int(v) for v in out]))
        res["out"] = [int(v) for v in out]
        return res

    def debug_corrupt(self, what, a, b=0, x=0.0):
        """TESTS ONLY (bslv_poly_debug_corrupt): 0 delete edge number a, 1 append edge (a, b), 2 drop the last entry of element a's
        incidence list, 3 add x to coordinate b of element a"""
        f = self.lib.bslv_poly_debug_corrupt
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
        check(f(self.h, int(what), int(a), int(b), float(x)))

    def counts(self):
        L, h = self.lib, self.h
        return dict(nprimal=L.bslv_poly_nprimal(h), ndual=L.bslv_poly_ndual(h), nedges=L.bslv_poly_nedges(h),
                    pair_tests=L.bslv_poly_pair_tests(h), new_vertices=L.bslv_poly_new_vertices(h))

    def dump(self):
        L, h, d = self.lib, self.h, self.d
        nv, nf = L.bslv_poly_nprimal(h), L.bslv_poly_ndual(h)
        pu, pi, ps = (np.zeros(nv, np.uint8) for _ in range(3))
        X = np.zeros((nv, d))
        check(L.bslv_poly_get_primal(h, pu.ctypes.data, pi.ctypes.data, ps.ctypes.data, X.ctypes.data))
        du, di = np.zeros(nf, np.uint8), np.zeros(nf, np.uint8)
        Y = np.zeros((nf, d))
        check(L.bslv_poly_get_dual(h, du.ctypes.data, di.ctypes.data, Y.ctypes.data))
        E = np.zeros((L.bslv_poly_nedges(h), 2), np.int32)
        check(L.bslv_poly_get_edges(h, E.ctypes.data))
        I = np.zeros((L.bslv_poly_ninc(h), 2), np.int32)
        check(L.bslv_poly_get_inc(h, I.ctypes.data))
        DE = np.zeros((L.bslv_poly_ndual_edges(h), 2), np.int32)
        check(L.bslv_poly_get_dual_edges(h, DE.ctypes.data))
        return dict(d=d, pu=pu, pi=pi, ps=ps, X=X, du=du, di=di, Y=Y, E=E, I=I, DE=DE)
