"""CPU: the impairment sweep's host side (tools/impairment_sweep.py): the summary of the per-channel words, the rank launcher, the torch
fallback of the gather with 32-byte words (gloo worlds of 2 and 8), and the numpy layouts of m17_impairment / m17_chan_stat."""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import m17hip
from m17hip import dist as mdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "impairment_sweep.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import impairment_sweep  # noqa: E402


def _words(rows):
    return np.array(rows, dtype=m17hip.CHAN_STAT_DTYPE)


def _points():
    return np.array([(0.0, 100.0, 0.0, 1.0), (800.0, 800.0, 1000.0, 0.5), (4000.0, 4000.0, -2500.0, 1.0)], dtype=m17hip.IMPAIRMENT_DTYPE)


def test_summarise_hand_built_words():
    #         channel point bits errors synced frames evm flags
    w = _words([(0, 0, 1000, 10, 1, 5, 0.25, 1),
                (3, 0, 3000, 0, 1, 6, 0.75, 1),
                (6, 0, 0, 0, 0, 2, 9.0, 0),        # not counting; its EVM is not valid
                (1, 1, 500, 50, 0, 3, 0.5, 1),
                (4, 1, 0, 0, 0, 0, 0.125, 1),      # not counting, EVM valid
                (7, 1, 2000, 20, 1, 4, 0.0, 0),    # counting, EVM not valid
                (2, 2, 0, 0, 0, 0, 0.0, 0)])       # nothing at all
    s = impairment_sweep.summarise(w, _points())
    assert len(s) == 3
    a, b, c = s
    assert (a["sigma"], a["tail_sigma"], a["dc"], a["gain"]) == (0.0, 100.0, 0.0, 1.0)
    assert a["channels"] == 3 and a["counting"] == 2 and a["synced"] == 2 and a["frames"] == 13
    assert a["bits"] == 4000 and a["errors"] == 10
    assert a["ber_pooled"] == 10 / 4000
    assert a["ber_mean"] == pytest.approx((0.01 + 0.0) / 2, abs=0, rel=1e-15)
    assert a["ber_worst"] == 0.01
    assert a["evm_median"] == 0.5 and a["evm_mean"] == 0.5 and a["evm_valid"] == 2
    assert (b["sigma"], b["dc"], b["gain"]) == (800.0, 1000.0, 0.5)
    assert b["channels"] == 3 and b["counting"] == 2 and b["synced"] == 1 and b["frames"] == 7
    assert b["bits"] == 2500 and b["errors"] == 70 and b["ber_pooled"] == 70 / 2500
    assert b["ber_mean"] == pytest.approx((0.1 + 0.01) / 2, abs=0, rel=1e-15) and b["ber_worst"] == 0.1
    assert b["evm_median"] == 0.3125 and b["evm_mean"] == 0.3125 and b["evm_valid"] == 2
    assert c["channels"] == 1 and c["counting"] == 0 and c["bits"] == 0
    assert c["ber_pooled"] is None and c["ber_mean"] is None and c["ber_worst"] is None
    assert c["evm_median"] is None and c["evm_mean"] is None and c["evm_valid"] == 0
    json.dumps(s)   # plain JSON


def test_summarise_is_order_free():
    rng = np.random.default_rng(5)
    n, P = 300, 7
    w = np.zeros(n, dtype=m17hip.CHAN_STAT_DTYPE)
    w["channel"] = np.arange(n)
    w["point"] = w["channel"] % P
    w["bits"] = rng.integers(0, 5000, n)
    w["errors"] = rng.integers(0, 50, n)
    w["evm"] = rng.random(n)
    w["flags"] = rng.integers(0, 2, n)
    pts = impairment_sweep.grid(sigmas=[0.0], dcs=[float(d) for d in range(P)])
    assert impairment_sweep.summarise(w, pts) == impairment_sweep.summarise(w[rng.permutation(n)], pts)


def test_default_grid_is_the_survey_grid():
    g = impairment_sweep.grid()
    assert g.size == 30
    assert sorted(set(g["noise_sigma"])) == [0.0, 400.0, 800.0, 1500.0, 2500.0, 4000.0]
    assert sorted(set(g["dc_offset"])) == [-2500.0, -1000.0, 0.0, 1000.0, 2500.0]
    assert set(g["gain"]) == {1.0}
    assert np.array_equal(g["tail_sigma"], np.maximum(g["noise_sigma"], 100.0))


def test_dry_launch_shows_eight_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, TOOL, "--gpus", "8", "--channels", "4096", "--check", "2", "--dry-launch"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    plan = json.loads(lines[0])["dry_launch"]
    assert [p["rank"] for p in plan] == list(range(8))
    assert len({p["env"]["MASTER_PORT"] for p in plan}) == 1
    assert len({json.dumps(p["env"], sort_keys=True) for p in plan}) == 8
    for r_, p in enumerate(plan):
        e = p["env"]
        assert e["RANK"] == e["LOCAL_RANK"] == str(r_) and e["WORLD_SIZE"] == "8" and e["MASTER_ADDR"] == "127.0.0.1"
        assert p["argv"][1] == TOOL and p["argv"][2:] == ["--gpus", "8", "--channels", "4096", "--check", "2"]


def _rank_words(lo, hi, P):
    w = np.zeros(hi - lo, dtype=m17hip.CHAN_STAT_DTYPE)
    w["channel"] = np.arange(lo, hi)
    w["point"] = w["channel"] % P
    w["bits"] = (w["channel"] * 37) % 4000
    w["errors"] = w["channel"] % 11
    w["synced"] = w["channel"] % 3 != 0
    w["frames"] = w["channel"] % 5
    w["evm"] = (w["channel"] % 97) / 128.0
    w["flags"] = w["channel"] % 13 != 0
    return w


C_TOTAL, P_TOTAL = 203, 30


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = mdist.shard_range(C_TOTAL, rank, world)
    mine = _rank_words(lo, hi, P_TOTAL)
    buf = torch.from_numpy(np.frombuffer(mine.tobytes(), dtype=np.uint8).copy()) if mine.size else torch.zeros(32, dtype=torch.uint8)
    out, counts = mdist.gather_records(buf, mine.size, rec_bytes=32)
    assert tuple(out.shape) == (C_TOTAL, 32)
    np.save(os.path.join(outdir, f"rank{rank}.npy"), out.numpy())
    np.save(os.path.join(outdir, f"counts{rank}.npy"), np.array(counts))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_gloo_gather_of_sweep_words(tmp_path, world):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    whole = _rank_words(0, C_TOTAL, P_TOTAL)
    pts = impairment_sweep.grid()
    for r in range(world):
        got = np.frombuffer(np.load(os.path.join(tmp_path, f"rank{r}.npy")).tobytes(), dtype=m17hip.CHAN_STAT_DTYPE)
        assert got.tobytes() == whole.tobytes(), r
        counts = np.load(os.path.join(tmp_path, f"counts{r}.npy"))
        assert counts.tolist() == [hi - lo for lo, hi in (mdist.shard_range(C_TOTAL, k, world) for k in range(world))]
        assert impairment_sweep.summarise(got, pts) == impairment_sweep.summarise(whole, pts)


def test_gather_records_default_is_the_frame_record():
    buf = torch.arange(3 * 64, dtype=torch.int64).to(torch.uint8)
    out, counts = mdist.gather_records(buf, 3)
    assert tuple(out.shape) == (3, 64) and counts == [3]
    out, counts = mdist.gather_records(buf, 5, rec_bytes=32)
    assert tuple(out.shape) == (5, 32) and counts == [5]


def test_numpy_layouts_match_the_header():
    assert m17hip.IMPAIRMENT_DTYPE.itemsize == m17hip.CHAN_STAT_DTYPE.itemsize == 32
    hdr = open(os.path.join(ROOT, "include", "m17hip.h")).read()

    def c_fields(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            toks = decl.replace(",", " , ").split()
            if not toks:
                continue
            ctype, names = toks[0], [t for t in toks[1:] if t != ","]
            out += [(n, ctype) for n in names]
        return out

    sizes = {"double": 8, "uint32_t": 4, "float": 4}
    kinds = {"double": "f", "uint32_t": "u", "float": "f"}
    for name, dt in (("m17_impairment", m17hip.IMPAIRMENT_DTYPE), ("m17_chan_stat", m17hip.CHAN_STAT_DTYPE)):
        fields = c_fields(name)
        assert [n for n, _ in fields] == list(dt.names), name
        off = 0
        for n, ctype in fields:
            assert dt.fields[n][1] == off, (name, n)
            assert dt.fields[n][0].itemsize == sizes[ctype] and dt.fields[n][0].kind == kinds[ctype], (name, n)
            off += sizes[ctype]
        assert off == 32
    assert "M17HIP_MAX_SWEEP_POINTS 4096u" in hdr and m17hip.MAX_SWEEP_POINTS == 4096
