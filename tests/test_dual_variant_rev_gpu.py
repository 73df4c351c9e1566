"""GPU: the dual variant of Benson's algorithm (phase2_dual -a dual, phase1_dual -A dual) with the LP engine in the REVISED form.

Both halves are built on batches of P1(w) LPs that differ in their objective (bslv_lpq_solve_batch_obj).  The engine chooses the
revised form by itself only for problems whose tableaux would be 4 GiB and more; BSLV_LP_REV=1 forces it here, on problems small
enough to compare: through the Python layer against the tableau form, through the command line against the hybrid goldens."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bensolve_amd import synth
from bensolve_amd.vlp import solve_primal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
EXDIR = os.path.join(ROOT, "tests", "golden", "ex")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hybrid.npz"))
EX_TOL = 1e-9


def _dual_run(monkeypatch, prob, rev, **env):
    monkeypatch.setenv("BSLV_LP_REV", rev)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = solve_primal(prob, bounded=True, batch=32, eps_benson_phase2=1e-9, alg_phase2="dual")
    for k in env:
        monkeypatch.delenv(k)
    return out


COVERING = [(30, 15, 3, 5, 1), (40, 20, 4, 9, 1), (25, 12, 3, 8, -1)]


def _covering(m, n, q, seed, sense):
    prob = synth.covering_vlp(m, n, q, seed)
    if sense == -1:
        prob["P"] = -prob["P"]; prob["optdir"] = -1
    return prob


@pytest.mark.parametrize("m,n,q,seed,sense", COVERING)
def test_dual_variant_revised_form_gives_the_images_of_the_tableau_form(monkeypatch, m, n, q, seed, sense):
    """phase2_dual with the revised form against phase2_dual with the tableau form: same vertices and directions of both images,
    same incidence and adjacency (exact sets)"""
    import poly_harness as ph
    prob = _covering(m, n, q, seed, sense)
    a = _dual_run(monkeypatch, prob, "0")
    b = _dual_run(monkeypatch, prob, "1")
    assert a["status"] == b["status"] == "optimal", (a["message"], b["message"])
    ca, cb = ph.canonical(a["dump"], decimals=6), ph.canonical(b["dump"], decimals=6)
    ph.assert_benson_results_agree(cb, ca)


def test_dual_variant_retries_an_undefined_lp(monkeypatch):
    """An LP of phase2_dual that comes back UNDEFINED (BSLV_LP_OBJ_UNDEFINED=2:0: LP 0 of the first batch of PART 2, as when the
    revised form's pivot cross-check gives an LP up) is solved again from slot 0: the run ends with the images of the run without it"""
    import poly_harness as ph
    prob = _covering(30, 15, 3, 5, 1)
    a = _dual_run(monkeypatch, prob, "1")
    b = _dual_run(monkeypatch, prob, "1", BSLV_LP_OBJ_UNDEFINED="2:0")
    assert a["status"] == b["status"] == "optimal", (a["message"], b["message"])
    ph.assert_benson_results_agree(ph.canonical(b["dump"], decimals=6), ph.canonical(a["dump"], decimals=6))


def _read_img(path):
    a = np.array([[float(x) for x in l.split()] for l in open(path).read().strip().splitlines()])
    t, X = a[:, 0].astype(int), a[:, 1:]
    for i in np.nonzero(t == 0)[0]:
        X[i] /= np.abs(X[i]).max()
    key = np.round(X, 6) + 0.0
    o = np.lexsort([key[:, j] for j in range(X.shape[1] - 1, -1, -1)] + [1 - t])
    return t[o], X[o]


def _rev_env():
    return dict(os.environ, BSLV_LP_REV="1")


@pytest.mark.parametrize("alg1,alg", [("primal", "dual"), ("dual", "dual"), ("dual", "primal")])
@pytest.mark.parametrize("ex", ["ex01", "ex05", "ex06", "ex08", "ex11"])
def test_cli_dual_variants_in_the_revised_form_match_hybrid_goldens(tmp_path, ex, alg1, alg):
    """-A dual / -a dual with the revised form: the committed outputs of the hybrid at 1e-9, as test_cli_gpu.py checks the default"""
    base = os.path.join(tmp_path, ex)
    r = subprocess.run([CLI, os.path.join(EXDIR, ex + ".vlp"), "-m", "2", "-B", "64", "-A", alg1, "-a", alg, "-o", base],
                       capture_output=True, text=True, timeout=600, env=_rev_env())
    assert r.returncode == 0, r.stdout + r.stderr
    for side in ("p", "d"):
        t, X = _read_img(base + "_img_%s.sol" % side)
        gt, gX = _read_img_gold(ex, side)
        assert np.array_equal(t, gt), (ex, side, r.stdout)
        np.testing.assert_allclose(X, gX, rtol=EX_TOL, atol=EX_TOL)


def _read_img_gold(ex, side):
    t, X = GOLD["%s/%s_type" % (ex, side)], GOLD["%s/%s" % (ex, side)].copy()
    for i in np.nonzero(t == 0)[0]:
        X[i] /= np.abs(X[i]).max()
    key = np.round(X, 6) + 0.0
    o = np.lexsort([key[:, j] for j in range(X.shape[1] - 1, -1, -1)] + [1 - t])
    return t[o], X[o]


def test_cli_solution_files_of_the_dual_variant_in_the_revised_form(tmp_path):
    """-s -a dual with the revised form: an x for every element of the upper image, a dual solution (u, w) for every vertex of the
    lower image (u from the row duals of the P1(w) LP), with the certificate checks of test_cli_solution_files"""
    m, n, q = 30, 15, 3
    prob = synth.covering_vlp(m, n, q, 5)
    path = os.path.join(tmp_path, "prob.vlp")
    synth.write_vlp(prob, path)
    base = os.path.join(tmp_path, "hip")
    r = subprocess.run([CLI, path, "-s", "-m", "1", "-B", "32", "-a", "dual", "-o", base, "-b"], capture_output=True, text=True, timeout=300, env=_rev_env())
    assert r.returncode == 0, r.stdout + r.stderr
    load = lambda suf: np.array([[float(x) for x in l.split()] for l in open(base + suf).read().strip().splitlines()])
    img, pre = load("_img_p.sol"), load("_pre_img_p.sol")
    assert pre.shape == (len(img), n)
    pts = img[:, 0] == 1
    assert pts.sum() >= 3
    X = pre[pts]
    np.testing.assert_allclose(X @ prob["P"].T, img[pts][:, 1:], rtol=1e-7, atol=1e-7)
    assert np.all(X >= -1e-9) and np.all(X @ prob["A"].T >= 1 - 1e-7)
    dirs = pre[~pts]
    assert np.all(dirs >= -1e-9) and np.all(dirs @ prob["A"].T >= -1e-7)
    imd, prd = load("_img_d.sol"), load("_pre_img_d.sol")
    assert prd.shape == (len(imd), m + q)
    vd = imd[:, 0] == 1
    U, W, Ys = prd[vd][:, :m], prd[vd][:, m:], imd[vd][:, 1:]
    assert np.all(U >= -1e-9)
    np.testing.assert_allclose(W[:, :-1], Ys[:, :-1], rtol=0, atol=1e-8)
    np.testing.assert_allclose(W.sum(axis=1), 1.0, rtol=0, atol=1e-8)
    np.testing.assert_allclose(U.sum(axis=1), Ys[:, -1], rtol=1e-7, atol=1e-7)
    assert np.all(U @ prob["A"] <= W @ prob["P"] + 1e-7)


@pytest.mark.skipif(not os.environ.get("BSLV_RUN_EX07_DUAL_REV"), reason="ex07 with -a dual in the revised form: set BSLV_RUN_EX07_DUAL_REV=1")
def test_cli_ex07_dual_variant_in_the_revised_form_is_certified(tmp_path):
    vlp = os.path.join(EXDIR, "ex07.vlp")
    base = os.path.join(tmp_path, "ex07")
    r = subprocess.run([CLI, vlp, "-e", "0.05", "-s", "-a", "dual", "-o", base], capture_output=True, text=True, timeout=900, env=_rev_env())
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    c = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_solution.py"), vlp, base, "0.05"], capture_output=True, text=True, timeout=900)
    cert = json.loads(c.stdout.strip().splitlines()[-1])
    assert c.returncode == 0 and cert["ok"], cert
