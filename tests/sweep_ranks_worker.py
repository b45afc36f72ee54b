"""One RANK of the N > 1 tests of m17hip_gather_sweep_stats (tests/test_gpu_sweep_ranks.py starts N of these on the ONE GPU of a test box, with
tests/fake_rccl first in LD_LIBRARY_PATH so that the product's dlopen("librccl.so.1") binds the test double).

    sweep_ranks_worker.py <rank> <world> <dir>

The rank works through its (uneven) shard in slabs of SLAB channels — synthesis of the impairment grid, a fresh run, the sweep words — and
gathers its words to rank 0; then the failure agreement (m17hip_tune key 30 = 1 on one rank).  Every rank writes <dir>/result<rank>.json and
rank 0 its gathered words as <dir>/words.npy.  No torch in this process: torch carries an RCCL of its own and the product would bind that one.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "m17-cxx-demod_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import m17hip  # noqa: E402
import oracle_lib as ol  # noqa: E402  (generator parameters only: the layout of m17_synth_params)
import impairment_sweep  # noqa: E402  (the grid)

CT, T, SLAB = 150, 24000, 25
SHARDS = {2: [0, 70, 150], 4: [0, 31, 75, 112, 150]}


def base():
    return ol.gen_params(seed=2024, kind=0, n_frames=T // 1920 + 2, lead_in=3072, lead_sigma=40000.0, total=T)


def new_comm(ctx, rank, world, d, n):
    """Collective: rank 0 draws an id and leaves it in a file."""
    path = os.path.join(d, f"id{n}")
    if rank == 0:
        with open(path + ".tmp", "wb") as f:
            f.write(m17hip.comm_get_id())
        os.rename(path + ".tmp", path)
    t0 = time.time()
    while not os.path.exists(path):
        assert time.time() - t0 < 300, "no communicator id from rank 0"
        time.sleep(0.02)
    return m17hip.Comm(ctx, open(path, "rb").read(), rank, world)


def gather_raw(ctx, comm, words, world, root=0, capacity=4 * CT):
    counts = np.zeros(world, dtype=np.uint64)
    total = C.c_uint64(0)
    out = np.zeros(capacity, dtype=m17hip.CHAN_STAT_DTYPE) if comm.rank == root else None
    code = ctx.lib.m17hip_gather_sweep_stats(ctx.h, comm.h, C.c_int(root), words.ctypes.data_as(C.c_void_p), C.c_uint64(words.size),
                                             None if out is None else out.ctypes.data_as(C.c_void_p), C.c_uint64(capacity if out is not None else 0),
                                             counts.ctypes.data_as(C.c_void_p), C.byref(total))
    return code, (out[: min(total.value, capacity)] if out is not None else None), [int(v) for v in counts], int(total.value)


def main():
    assert "torch" not in sys.modules
    rank, world, d = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    lo, hi = SHARDS[world][rank], SHARDS[world][rank + 1]
    res = {}
    ctx = m17hip.Context(SLAB, T)
    try:
        ctx.tune(6, 1)
        ctx.tune(31, 20000)   # every wait of the gather bounded at 20 s
        pts = impairment_sweep.grid()
        words, slabs = [], 0
        for s0 in range(lo, hi, SLAB):
            cs = min(SLAB, hi - s0)
            ctx.set_channel_base(s0)
            ctx.synth_sweep(base(), pts, cs, T, chan0=s0)
            ctx.reset(); ctx.run()
            words.append(ctx.sweep_stats(pts.size, cs))
            slabs += 1
        mine = np.concatenate(words)
        res["slabs"] = slabs
        comm = new_comm(ctx, rank, world, d, 1)
        maps = open("/proc/self/maps").read()
        res["bound_fake"] = "tests/fake_rccl/librccl.so.1" in maps
        code, out, counts, total = gather_raw(ctx, comm, mine, world)
        res["basic"] = {"code": code, "counts": counts, "total": total}
        if rank == 0:
            np.save(os.path.join(d, "words.npy"), out)
        clean = None if out is None else out.tobytes()
        code, out, counts, total = gather_raw(ctx, comm, mine, world, capacity=7)   # a truncated destination on the root
        res["trunc"] = {"code": code, "total": total, "head_ok": (out.tobytes() == clean[: 7 * 32]) if rank == 0 else None}
        faults = {}
        for f in (1, 0):   # this rank's upload of its words fails: its own code there, ECOMM elsewhere, and the communicator delivers again
            if rank == f:
                ctx.tune(30, 1)
            t0 = time.time()
            code, _, _, _ = gather_raw(ctx, comm, mine, world)
            ctx.tune(30, 0)
            code2, out, counts, total = gather_raw(ctx, comm, mine, world)
            faults[f"1@{f}"] = {"code": code, "s": time.time() - t0, "after": code2, "after_ok": (out.tobytes() == clean) if rank == 0 else None}
        res["faults"] = faults
        comm.close()
        res["done"] = True
    finally:
        with open(os.path.join(d, f"result{rank}.json"), "w") as f:
            json.dump(res, f)
        ctx.close()


if __name__ == "__main__":
    main()
