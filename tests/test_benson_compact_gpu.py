"""GPU: the compaction trigger of the Benson driver (bslv_benson_set_compact, BSLV_POLY_COMPACT; include/bslv_hip.h).

The trajectory of a run does not depend on the names of the elements, so a run with the trigger on -- here with f = 0.05 and
min_slots = 1, which compacts after almost every apply -- solves the same LPs, applies the same cuts and ends with the same sets,
bit for bit, as the run with the trigger off; only nprimal is smaller.  Against the CPU oracle the runs are compared as
test_benson_gpu.py compares these sizes (assert_benson_results_agree at its defaults; that file documents no allowance for them)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import poly_harness as ph
from bensolve_amd import synth
from bensolve_amd.benson import BensonEngine, PipelinedStepper

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "bensolve_amd", "csrc", "bensolve_hip")
F, MIN = 0.05, 1
PROBLEMS = {"covering": (synth.covering_vlp, (60, 30, 3, 7), 64), "degenerate": (synth.degenerate_vlp, (60, 30, 4, 3), 64)}


def _finish(eng):
    eng.poly_call("dual_adjacency")
    d = eng.poly_dump()
    res = dict(can=ph.canonical(d, decimals=6), totals=eng.totals(), stats=eng.compact_stats(), nprimal=len(d["pu"]), live=int(d["pu"].sum()),
               check=eng.poly_call("check")["clean"])
    eng.close()
    return res


@functools.lru_cache(maxsize=None)
def run(which, how):
    """how: "off", "on" (set_compact) or "env" (BSLV_POLY_COMPACT when the engine is created); to termination.  Read-only for its users."""
    gen, args, batch = PROBLEMS[which]
    old = os.environ.pop("BSLV_POLY_COMPACT", None)
    if how == "env":
        os.environ["BSLV_POLY_COMPACT"] = "%g:%d" % (F, MIN)
    try:
        eng = BensonEngine(gen(*args), eps=1e-9, pool_slots=max(4 * batch, 64))
    finally:
        os.environ.pop("BSLV_POLY_COMPACT", None)
        if old is not None:
            os.environ["BSLV_POLY_COMPACT"] = old
    if how == "on":
        eng.set_compact(F, MIN)
    assert eng.start() == 0
    eng.run(batch)
    return _finish(eng)


@functools.lru_cache(maxsize=None)
def oracle(which):
    import oracle_api
    gen, args, _ = PROBLEMS[which]
    rc, fp, st = oracle_api.benson_phase2_primal(gen(*args), eps=1e-9)
    assert rc == 0
    fp.dual_adjacency()
    exp = ph.canonical(fp.dump(), decimals=6)
    fp.close()
    return exp


@pytest.mark.parametrize("which", list(PROBLEMS))
def test_on_equals_off(which):
    on, off = run(which, "on"), run(which, "off")
    print("%s: off %d slots (%d live), on %d slots; %s" % (which, off["nprimal"], off["live"], on["nprimal"], on["stats"]))
    assert on["totals"] == off["totals"]
    ph.assert_same(on["can"], off["can"], rtol=0, atol=0)
    ph.assert_benson_results_agree(on["can"], oracle(which))
    assert off["stats"]["out"] == [0, 0, 0, 0]
    assert on["stats"]["compactions"] >= 1 and on["stats"]["slots_removed"] > 0
    assert on["nprimal"] < off["nprimal"] and on["live"] == off["live"]
    assert on["check"] and off["check"]


def test_the_environment_switch(monkeypatch):
    env, on = run("covering", "env"), run("covering", "on")
    for k in ("compactions", "slots_removed", "pool_removed"):
        assert env["stats"][k] == on["stats"][k], k
    ph.assert_same(env["can"], on["can"], rtol=0, atol=0)
    # a homogeneous engine takes the switch too, and its result does not change
    from test_benson_certify_gpu import _homogeneous_engine
    res = {}
    for how in ("off", "env"):
        if how == "env":
            monkeypatch.setenv("BSLV_POLY_COMPACT", "%g:%d" % (F, MIN))
        else:
            monkeypatch.delenv("BSLV_POLY_COMPACT", raising=False)
        eng = _homogeneous_engine(synth.covering_vlp(30, 15, 3, 5), 256)
        assert eng.start() == 0
        for _ in range(4):                                    # (BATCH and STEPS of test_benson_certify_gpu.py)
            nl, nt = eng.collect(32)
            rec, _, _ = eng.solve_local(nl)
            eng.apply(rec)
        res[how] = _finish(eng)
    print("homogeneous:", res["env"]["stats"], res["off"]["nprimal"], "->", res["env"]["nprimal"])
    # (the cone of this problem keeps its q + 1 elements through these iterations: the engine takes the switch, and has nothing to remove)
    assert res["off"]["stats"]["compactions"] == 0 and res["env"]["nprimal"] == res["env"]["live"]
    assert res["env"]["totals"] == res["off"]["totals"]
    ph.assert_same(res["env"]["can"], res["off"]["can"], rtol=0, atol=0)


def test_preimages_follow_the_renumbering(tmp_path):
    """bensolve_hip -s -B 16 on the (30, 15, 3, 5) covering problem, plain and under BSLV_POLY_COMPACT: the same .sol files byte for byte"""
    path = os.path.join(tmp_path, "prob.vlp")
    synth.write_vlp(synth.covering_vlp(30, 15, 3, 5), path)
    files = {}
    for how in ("plain", "compact"):
        base = os.path.join(tmp_path, how)
        env = dict(os.environ)
        env.pop("BSLV_POLY_COMPACT", None)
        if how == "compact":
            env["BSLV_POLY_COMPACT"] = "%g:%d" % (F, MIN)
        r = subprocess.run([CLI, path, "-s", "-m", "1", "-B", "16", "-o", base], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        files[how] = {f[len(how):]: open(os.path.join(tmp_path, f), "rb").read() for f in sorted(os.listdir(tmp_path)) if f.startswith(how) and f.endswith(".sol")}
    assert len(files["plain"]) >= 4 and set(files["plain"]) == set(files["compact"]), (sorted(files["plain"]), sorted(files["compact"]))
    for suffix, blob in files["plain"].items():
        assert blob == files["compact"][suffix], suffix
    assert len(files["plain"]["_pre_img_p.sol"]) > 0


def test_pipelined_mode():
    gen, args, batch = PROBLEMS["covering"]
    res = {}
    for how in ("off", "on"):
        eng = BensonEngine(gen(*args), eps=1e-9, pool_slots=max(8 * batch, 128))
        if how == "on":
            eng.set_compact(F, MIN)
        assert eng.start() == 0
        PipelinedStepper(eng, batch).run()
        res[how] = _finish(eng)
    print("pipelined: %d compactions (%s)" % (res["on"]["stats"]["out"][0], res["on"]["stats"]))
    ph.assert_same(res["on"]["can"], res["off"]["can"], rtol=0, atol=0)
    assert res["on"]["check"]


def _rank_main(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    eng = BensonEngine(synth.covering_vlp(30, 15, 3, 5), eps=1e-9, pool_slots=512)
    eng.set_compact(F, MIN)
    assert eng.start() == 0
    steps = 0
    while True:
        s = eng.step_distributed(32, dist, torch.device("cpu"))
        steps += 1
        if s["n_total"] == 0 or steps > 500:
            break
    eng.poly_call("dual_adjacency")
    d = eng.poly_dump()
    st = eng.compact_stats()["out"]
    eng.close()
    np.savez(out, stats=np.array(st[:3], np.int64), **d)
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu(tmp_path):
    """the worker pattern of test_benson_gpu.test_two_ranks_match_single with the trigger on in both ranks: the decision reads replicated
    state only, so both compact after the same applies, stay bit-identical and end with the sets of the single-rank run"""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    outs = [os.path.join(tmp_path, "rank%d.npz" % r) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "rank", str(r), "2", str(port), outs[r]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    logs, codes = [], []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for o in procs:
                o.kill()
            logs.append(p.communicate()[0])
        codes.append(p.returncode)
        if p.returncode != 0:                                 # a rank that failed leaves the other waiting for it: end it now
            for o in procs:
                if o.poll() is None:
                    o.kill()
    assert codes == [0, 0], (codes, [l[-1500:] for l in logs])
    d0, d1 = (dict(np.load(o)) for o in outs)
    for k in ("stats", "pu", "pi", "E", "I", "X", "Y", "du"):
        assert np.array_equal(d0[k], d1[k]), "replicas diverged in " + k
    print("two ranks: compactions, slots removed, pool words removed =", d0["stats"].tolist())
    assert d0["stats"][0] >= 1 and d0["stats"][1] > 0
    eng = BensonEngine(synth.covering_vlp(30, 15, 3, 5), eps=1e-9, pool_slots=512)
    assert eng.start() == 0
    eng.run(32)
    single = _finish(eng)
    ph.assert_benson_results_agree(ph.canonical(d0, decimals=6), single["can"])


def test_arguments():
    eng = BensonEngine(synth.covering_vlp(12, 6, 2, 3), eps=1e-9, pool_slots=64)
    f = eng.lib.bslv_benson_set_compact
    f.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_long]
    for bad in (-0.1, 1.5, float("nan")):
        assert f(eng.h, bad, -1) == 2, bad                    # BSLV_E_ARG
    assert eng.start() == 0
    eng.run(4)
    assert eng.compact_stats()["out"] == [0, 0, 0, 0]         # the switch stayed off
    assert f(None, 0.5, -1) == 2 and f(eng.h, 1.0, -1) == 0 and f(eng.h, 0.0, 0) == 0
    eng.close()


if __name__ == "__main__" and sys.argv[1:2] == ["rank"]:
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
