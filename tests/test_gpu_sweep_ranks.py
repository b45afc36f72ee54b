"""m17hip_gather_sweep_stats with MORE THAN ONE RANK, on the one GPU of a test box, through the librccl test double (tests/fake_rccl, found
by the product's dlopen in the CHILD processes only, as tests/test_gpu_gather_ranks.py does): uneven shards, each worked through in several
slabs, gathered to rank 0 == the words of one run over the whole channel set; the failure agreement of key 30."""
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import m17hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_rccl")
WORKER = os.path.join(ROOT, "tests", "sweep_ranks_worker.py")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweep_ranks_worker as W  # noqa: E402  (sizes, shards, generator parameters: the same as the workers')
import impairment_sweep  # noqa: E402

EHIP, ETRUNC, ECOMM = -2, -6, -7


def _whole():
    pts = impairment_sweep.grid()
    c = m17hip.Context(W.CT, W.T)
    c.tune(6, 1)
    c.synth_sweep(W.base(), pts, W.CT, W.T, chan0=0)
    c.reset(); c.run()
    w = c.sweep_stats(pts.size, W.CT)
    c.close()
    return w


def _run_ranks(tmp_path, world, wall_s=600):
    if not os.path.exists(os.path.join(FAKE_DIR, "librccl.so.1")):
        pytest.fail("tests/fake_rccl/librccl.so.1 is not built (__graft_entry__.build() / make -C tests/fake_rccl)")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = FAKE_DIR + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    env["M17_FAKE_RCCL_LOG"] = str(tmp_path / "fake")
    env["M17_FAKE_RCCL_TIMEOUT_MS"] = "60000"
    env.pop("M17_FAKE_RCCL_ON_TIMEOUT", None)
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(tmp_path)], env=env, stderr=open(tmp_path / f"err{r}.txt", "w"))
             for r in range(world)]
    t0 = time.time()
    try:
        while any(p.poll() is None for p in procs):
            if time.time() - t0 > wall_s:
                pytest.fail(f"ranks still running after {wall_s} s: " + str([p.poll() for p in procs]))
            time.sleep(0.1)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for f in glob.glob("/dev/shm/m17fakerccl_*"):
            try:
                os.unlink(f)
            except OSError:
                pass
    errs = [open(tmp_path / f"err{r}.txt").read() for r in range(world)]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r}: exit {p.returncode}\n{errs[r][-3000:]}"
    res = [json.load(open(tmp_path / f"result{r}.json")) for r in range(world)]
    assert all(x.get("done") for x in res)
    for e in errs:
        assert "FAKE_RCCL_SIZE_MISMATCH" not in e
    return res


@pytest.mark.parametrize("world", [2, 4])
def test_sweep_words_gathered_over_ranks_equal_one_run(tmp_path, world):
    res = _run_ranks(tmp_path, world)
    sh = W.SHARDS[world]
    per_rank = [sh[r + 1] - sh[r] for r in range(world)]
    assert len(set(per_rank)) > 1   # uneven shards
    whole = _whole()
    assert whole.size == W.CT and (whole["frames"] > 0).mean() >= 0.9
    assert np.load(tmp_path / "words.npy").tobytes() == whole.tobytes()
    for r in range(world):
        assert res[r]["bound_fake"] is True, "the product did not bind the test double"
        assert res[r]["slabs"] > 1
        b = res[r]["basic"]
        assert b["code"] == 0 and b["counts"] == per_rank and b["total"] == W.CT, (r, b)
        t = res[r]["trunc"]
        assert t["total"] == W.CT and t["code"] == (ETRUNC if r == 0 else 0) and t["head_ok"] in (True, None), (r, t)
        for f in (1, 0):
            got = res[r]["faults"][f"1@{f}"]
            assert got["code"] == (EHIP if r == f else ECOMM), (f, r, got)
            assert got["after"] == 0 and got["after_ok"] in (True, None), (f, r, got)
            assert got["s"] < 20, (f, r, got)
