"""GPU: what a user takes away from bensolve_hip -s -- an x for every vertex and extreme direction of the upper image, a dual solution
(u, w) for every vertex of the lower image -- certified against the PROBLEM on general models (tests/vlp_general_cases.py: folded
singleton rows, rows and columns of every type, max problems, unbounded images, ordering cones by generators), in every variant that
produces them: primal and dual algorithm, tableau and revised LP form, presolve on and off, small batches (kept and parked
tableaux), compaction, dual phase 1.

Every run must (a) reproduce the images of the reference's driver (tests/golden/solutions.npz, sorted as test_cli_gpu.read_img sorts
them) to 1e-6, the bound of test_cli_gpu.test_cli_files_match_hybrid, and (b) pass tests/solution_certificate.py on EVERY row,
including the dual vertices on which the reference's own files fail (solutions.json: w_mismatch), each residual within
solution_certificate.bound: min(1e-7 scale, max(10 x the reference's recorded residual, 1e-9 scale))."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import solution_certificate as sc
import vlp_general_cases as gc
from bensolve_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
GOLD = np.load(os.path.join(HERE, "golden", "solutions.npz"))
META = json.load(open(os.path.join(HERE, "golden", "solutions.json")))
EPS = sc.DEFAULT_EPS
ENV_KEYS = ("BSLV_LP_REV", "BSLV_NO_PRESOLVE", "BSLV_POLY_COMPACT", "BSLV_CANONICAL_OBJ")


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """cli_run(case, alg, rev, args, env): one run of the command-line driver, -s -B 32 unless args name another batch, default eps.
    A run is made once and shared by the tests that read it; nobody changes it."""
    work = str(tmp_path_factory.mktemp("solutions"))
    done = {}

    def run(case, alg="primal", rev=0, args=(), env=()):
        key = (case, alg, rev, args, env)
        if key in done:
            return done[key]
        path = os.path.join(work, case + ".vlp")
        if not os.path.exists(path):
            synth.write_vlp(gc.CASES[case](), path)
        base = os.path.join(work, "_".join([case, alg, "rev%d" % rev] + [a.strip("-") for a in args] + [k for k, _ in env]))
        e = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
        e["BSLV_LP_REV"] = str(rev)
        e.update(dict(env))
        cmd = [CLI, path, "-s", "-m", "1", "-a", alg, "-o", base] + ([] if "-B" in args else ["-B", "32"]) + list(args)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=e)
        assert r.returncode == 0, ("exit status %d" % r.returncode, cmd, r.stdout[-2000:], r.stderr[-2000:])
        done[key] = sc.load_run(base)
        return done[key]
    return run


def assert_run(case, run, bounded=False):
    key = case + ("+b" if bounded else "")
    prob, meta = gc.CASES[case](), META[key]
    # (a) the images of the reference's driver
    for side in ("p", "d"):
        t, X, _ = sc.sorted_img(run["img_" + side])
        gt, gX, _ = sc.sorted_img(np.column_stack([GOLD[key + "/" + side + "_type"], GOLD[key + "/" + side]]))
        assert np.array_equal(t, gt), (key, side, len(t), len(gt))
        np.testing.assert_allclose(X, gX, rtol=1e-6, atol=1e-6, err_msg="%s img_%s" % (key, side))
    np.testing.assert_allclose(run["c"], GOLD[key + "/c"], rtol=1e-9, atol=1e-9)
    # (b) the certificate, on every row
    res = sc.certify(prob, run, EPS)
    scale = res["scale"]
    table = {k: (res[k]["value"], res[k]["row"], meta["residuals"][k]["value"], sc.bound(k, meta, scale)) for k in sc.CHECKS}
    report = "\n".join("%-20s measured %.3e (row %d)   reference %.3e   bound %.3e" % ((k,) + v) for k, v in table.items())
    print("%s scale %.4g, reference's w_mismatch %s\n%s" % (key, scale, meta["w_mismatch"], report))
    failed = [k for k, v in table.items() if not v[0] <= v[3]]
    assert not failed, "%s: %s\n%s" % (key, failed, report)
    return res


ALL = list(gc.CASES)


@pytest.mark.parametrize("rev", [0, 1], ids=["tableau", "revised"])
@pytest.mark.parametrize("alg", ["primal", "dual"])
@pytest.mark.parametrize("case", ALL)
def test_solution_is_certified(cli_run, case, alg, rev):
    assert_run(case, cli_run(case, alg, rev))


@pytest.mark.parametrize("case", gc.BOUNDED)
def test_bounded_option(cli_run, case):
    assert_run(case, cli_run(case, args=("-b",)), bounded=True)


@pytest.mark.parametrize("case", ALL)
def test_without_presolve(cli_run, case):
    """BSLV_NO_PRESOLVE=1 keeps the singleton rows in the LP: the same images to 1e-9, and both runs certify (the duals of the folded
    rows are rebuilt from reduced costs in one run and read from the tableau in the other)"""
    plain, folded = cli_run(case, env=(("BSLV_NO_PRESOLVE", "1"),)), cli_run(case)
    assert_run(case, plain)
    assert_run(case, folded)
    for side in ("img_p", "img_d"):
        (t1, X1, _), (t2, X2, _) = sc.sorted_img(plain[side]), sc.sorted_img(folded[side])
        assert np.array_equal(t1, t2)
        np.testing.assert_allclose(X1, X2, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", ["U3", "U4"])
def test_small_batches(cli_run, case):
    """-B 4: tableaux are kept for children and parked between batches; a pre-image must come from the slot of its own LP"""
    assert_run(case, cli_run(case, args=("-B", "4")))


def test_under_compaction(cli_run):
    """BSLV_POLY_COMPACT forced on as in test_benson_compact_gpu.py: the pre-image maps are re-keyed with the elements"""
    assert_run("B3max", cli_run("B3max", env=(("BSLV_POLY_COMPACT", "0.05:1"),)))


@pytest.mark.parametrize("case", ["U3-cone", "U4"])
def test_dual_phase1(cli_run, case):
    assert_run(case, cli_run(case, args=("-A", "dual")))


@pytest.mark.parametrize("alg", ["primal", "dual"])
def test_preimages_in_process(cli_run, alg):
    """vlp.solve_primal(..., preimages=True) on U3 returns what the command-line driver writes, row for row, after the writers' sign
    changes (u * optdir, w * c_dir); the dual algorithm's store is freed, and the old handle then has nothing stored"""
    from bensolve_amd import vlp
    from bensolve_amd._lib import load_library
    prob = gc.CASES["U3"]()
    m, n, q = prob["m"], prob["n"], prob["q"]
    files = cli_run("U3", alg, 0)
    old = os.environ.get("BSLV_LP_REV")
    os.environ["BSLV_LP_REV"] = "0"
    try:
        out = vlp.solve_primal(prob, batch=32, alg_phase2=alg, preimages=True)
        again = vlp.solve_primal(prob, batch=32, alg_phase2=alg, preimages=True)
    finally:
        os.environ.pop("BSLV_LP_REV")
        if old is not None:
            os.environ["BSLV_LP_REV"] = old
    assert out["status"] == "optimal"
    d = out["dump"]
    pu, pi, du, di = (d[k].astype(bool) for k in ("pu", "pi", "du", "di"))
    np.testing.assert_allclose(d["X"][pu & ~pi], files["img_p"][files["img_p"][:, 0] == 1][:, 1:], rtol=1e-13, atol=1e-10)
    rows_p = np.array([out["pre_p"].get(int(i), np.zeros(n)) for i in np.flatnonzero(pu)])
    np.testing.assert_allclose(rows_p, files["pre_p"], rtol=1e-13, atol=0)
    sign = np.concatenate([np.full(m, float(prob["optdir"])), np.full(q, float(out["c_dir"]))])
    rows_d = np.array([np.zeros(m + q) if di[k] or int(k) not in out["pre_d"] else out["pre_d"][int(k)] * sign for k in np.flatnonzero(du)])
    np.testing.assert_allclose(rows_d, files["pre_d"], rtol=1e-13, atol=0)
    assert all(int(i) in out["pre_p"] for i in np.flatnonzero(pu)) and all(int(k) in out["pre_d"] for k in np.flatnonzero(du & ~di))
    assert sorted(again["pre_p"]) == sorted(out["pre_p"]) and sorted(again["pre_d"]) == sorted(out["pre_d"])
    if alg == "dual":
        lib = load_library()
        buf = np.zeros(m + n + q)
        for handle in (out["lower_image_handle"], again["lower_image_handle"]):
            for f in (lib.bslv_dual_preimage_x, lib.bslv_dual_preimage_uw):
                for k in list(out["pre_p"])[:2] + list(out["pre_d"])[:2]:
                    assert f(ctypes.c_void_p(handle), k, buf.ctypes.data) == 1
