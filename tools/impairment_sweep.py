"""BASELINE configs[4]: an impairment sweep (AWGN, DC offset = FM frequency offset, gain) over C BERT channels x T samples,
EVM + BER per point, on N GPUs.

    python tools/impairment_sweep.py --gpus N [--channels 65536] [--samples 96000] [--slab 8192] [--sigmas ...] [--dcs ...] [--gains ...]
                                     [--check K] [--dry-launch] [--launch-timeout S]

Every channel carries one point of the grid: channel g takes point g % P (m17hip_synth_sweep_i16), so every contiguous shard carries every
point.  Each rank takes its shard (m17hip.dist.shard_range) and works through it in slabs of at most --slab channels: synthesis of the slab
on the device, a fresh run, one 32-byte word per channel (m17hip_sweep_stats: PRBS9 bits / errors / sync / BERT frames and SymbolEvm's
EVM).  The words go to rank 0 (m17hip_gather_sweep_stats, or m17hip.dist.gather_records over torch.distributed when the library's RCCL
communicator cannot be created), and rank 0 prints ONE JSON line: the summary of every point (`summarise`), the sizes, the gather path, the
rates, and the parity of --check K channels per point per rank against the CPU oracle (frame records, PRBS9 counts, diagnostics, bit for bit;
a mismatch makes the exit code non-zero).  With N > 1 and no launcher around it the tool starts its N ranks itself (tools/_toolslib.py)."""
import argparse
import json
import os
import sys
import time

# before anything initialises the HIP runtime (include/m17hip.h, m17hip_advice): 16 hardware queues, also over an inherited smaller value
if not os.environ.get("GPU_MAX_HW_QUEUES", "").isdigit() or int(os.environ["GPU_MAX_HW_QUEUES"]) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "m17-cxx-demod_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

SIGMAS = (0.0, 400.0, 800.0, 1500.0, 2500.0, 4000.0)
DCS = (0.0, 1000.0, -1000.0, 2500.0, -2500.0)
GAINS = (1.0,)
SEED = 779


def grid(sigmas=SIGMAS, dcs=DCS, gains=GAINS):
    """The sweep grid (IMPAIRMENT_DTYPE): every (sigma, dc, gain), the slab's tail as noisy as its burst but never silent (tail_sigma = max(sigma, 100))."""
    import m17hip
    pts = [(s, max(s, 100.0), d, g) for s in sigmas for d in dcs for g in gains]
    return np.array(pts, dtype=m17hip.IMPAIRMENT_DTYPE)


def _f(v):
    return None if v is None or not np.isfinite(v) else float(v)


def summarise(words, points):
    """Per point of `points` (IMPAIRMENT_DTYPE), from the gathered words (CHAN_STAT_DTYPE) alone: channels; channels counting (bits > 0);
    synced; BERT frames; sums of bits and errors; pooled BER (sum errors / sum bits); mean and worst channel BER over the counting
    channels; median and mean EVM over the words whose EVM is valid (flags bit 0).  None where there is nothing to average."""
    words = words[np.argsort(words["channel"], kind="stable")]   # (channel order: the same sums whatever order the words came in)
    out = []
    for p in range(len(points)):
        w = words[words["point"] == p]
        counting = w[w["bits"] > 0]
        ber = counting["errors"].astype(np.float64) / counting["bits"].astype(np.float64)
        evm = w["evm"][(w["flags"] & 1) != 0].astype(np.float64)
        bits, errors = int(w["bits"].astype(np.uint64).sum()), int(w["errors"].astype(np.uint64).sum())
        out.append({"sigma": float(points["noise_sigma"][p]), "tail_sigma": float(points["tail_sigma"][p]), "dc": float(points["dc_offset"][p]),
                    "gain": float(points["gain"][p]), "channels": int(w.size), "counting": int(counting.size), "synced": int((w["synced"] != 0).sum()),
                    "frames": int(w["frames"].astype(np.uint64).sum()), "bits": bits, "errors": errors,
                    "ber_pooled": errors / bits if bits else None,
                    "ber_mean": _f(ber.mean()) if ber.size else None, "ber_worst": _f(ber.max()) if ber.size else None,
                    "evm_median": _f(np.median(evm)) if evm.size else None, "evm_mean": _f(evm.mean()) if evm.size else None,
                    "evm_valid": int(evm.size)})
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=96000)
    ap.add_argument("--slab", type=int, default=8192, help="channels per synthesis + run (a rank's shard is worked through in slabs)")
    ap.add_argument("--sigmas", type=float, nargs="+", default=list(SIGMAS), help="AWGN sigmas (LSB)")
    ap.add_argument("--dcs", type=float, nargs="+", default=list(DCS), help="DC offsets (LSB)")
    ap.add_argument("--gains", type=float, nargs="+", default=list(GAINS))
    ap.add_argument("--check", type=int, default=0, help="channels per point per rank compared with the CPU oracle bit for bit")
    ap.add_argument("--dry-launch", action="store_true", help="with --gpus N > 1 and no launcher: print the N rank commands and exit")
    ap.add_argument("--launch-timeout", type=float, default=3600.0, help="with --gpus N > 1 and no launcher: seconds after which the ranks are stopped")
    return ap.parse_args(argv)


class Sweep:
    """One rank: its shard in slabs, its words, its share of the parity check."""

    def __init__(self, args):
        import m17hip
        import oracle_lib as ol
        from m17hip import dist as mdist
        self.m17hip, self.ol, self.mdist, self.args = m17hip, ol, mdist, args
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if self.world != args.gpus:
            sys.exit(f"impairment_sweep.py: WORLD_SIZE={self.world} but --gpus {args.gpus}")
        self.dist = None
        if self.world > 1:   # host-side rendezvous only (gloo on the CPU): the sweep's one exchange is the library's
            import torch.distributed as dist
            dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
            self.dist = dist
        self.points = grid(args.sigmas, args.dcs, args.gains)
        self.P = self.points.size
        self.C, self.T = args.channels, args.samples
        self.lo, self.hi = mdist.shard_range(self.C, self.rank, self.world)
        self.slab = max(1, min(args.slab, self.hi - self.lo))
        self.base = ol.gen_params(seed=SEED, kind=0, n_frames=self.T // 1920 + 2, lead_in=3072, lead_sigma=40000.0, noise_sigma=0.0, tail_sigma=100.0,
                                  total=self.T)
        self.ctx = m17hip.Context(self.slab, self.T, device=self.local_rank)
        self.ctx.tune(6, 1)
        # --check K: the first K channels of this shard on every point (all within its first K * P channels)
        first = [self.lo + (p - self.lo) % self.P for p in range(self.P)]
        self.check = sorted(g for f in first for g in range(f, self.hi, self.P)[: args.check])
        self.parity = {"checked": 0, "mismatches": 0}

    def _check(self, s0, cs, x, words):
        """The checked channels of the slab at s0 (x: its first rows as synthesised) against the oracle: records, PRBS9 counts, diagnostics."""
        ol = self.ol
        rows = [g - s0 for g in self.check if s0 <= g < s0 + cs]
        if not rows:
            return
        got, d = self.ctx.frames(), self.ctx.diag(cs)
        recs, counts, diags = ol.demod_batch(x[rows], cap=2 * (self.T // 1920 + 2) + 4, threads=min(16, os.cpu_count() or 1))
        for i, r in enumerate(rows):
            g = s0 + r
            bad = 0
            e = recs[i, : counts[i]].copy()
            e["channel"] = g
            bad += got[got["channel"] == g].tobytes() != e.tobytes()
            bert = e[e["frame_type"] == 5]
            bits, errs, sync = ol.bert_count(bert["payload"][:, :25]) if bert.size else (0, 0, False)
            w = words[r]
            bad += (int(w["bits"]), int(w["errors"]), bool(w["synced"]), int(w["frames"])) != (bits, errs, bool(sync), bert.size)
            bad += int(w["channel"]) != g or int(w["point"]) != g % self.P
            for f in ("evm", "deviation", "offset", "clock", "dcd_level"):
                bad += d[f][r].tobytes() != diags[f][i].tobytes()
            bad += w["evm"].tobytes() != diags["evm"][i].tobytes() and bool(w["flags"] & 1)
            self.parity["checked"] += 1
            self.parity["mismatches"] += bad > 0
            if bad:
                print(f"rank {self.rank}: channel {g} (point {g % self.P}) differs from the oracle", file=sys.stderr)

    def run(self):
        ctx, T = self.ctx, self.T
        words, t_synth, t_run = [], 0.0, 0.0
        n_check_rows = max([g - self.lo + 1 for g in self.check], default=0)
        t_start = time.perf_counter()
        for s0 in range(self.lo, self.hi, self.slab):
            cs = min(self.slab, self.hi - s0)
            ctx.set_channel_base(s0)
            t0 = time.perf_counter()
            ctx.synth_sweep(self.base, self.points, cs, T, chan0=s0)   # (complete when it returns)
            t1 = time.perf_counter()
            rows = min(cs, n_check_rows - (s0 - self.lo))
            x = ctx.download(channels=rows) if rows > 0 else None
            t2 = time.perf_counter()
            ctx.reset()
            ctx.run()
            w = ctx.sweep_stats(self.P, cs)   # (waits for the run and its payload work)
            t3 = time.perf_counter()
            t_synth += t1 - t0
            t_run += t3 - t2
            words.append(w)
            if x is not None:
                self._check(s0, cs, x, w)
        mine = np.concatenate(words) if words else np.zeros(0, dtype=self.m17hip.CHAN_STAT_DTYPE)
        t_loop = time.perf_counter() - t_start
        gathered, path = self.gather(mine)
        times = np.array([t_loop, t_synth, t_run, self.parity["checked"], self.parity["mismatches"]], dtype=np.float64)
        if self.dist is not None:
            import torch
            tt = torch.from_numpy(times[:3].copy())
            self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
            pc = torch.from_numpy(times[3:].copy())
            self.dist.all_reduce(pc, op=self.dist.ReduceOp.SUM)
            times = np.concatenate([tt.numpy(), pc.numpy()])
        self.ctx.close()
        if self.dist is not None:
            self.dist.destroy_process_group()
        if self.rank != 0:
            return int(times[4] > 0)
        assert gathered.size == self.C and np.array_equal(gathered["channel"], np.arange(self.C, dtype=np.uint32)), "gathered words out of order"
        samples = float(self.C) * self.T
        res = {"metric": "impairment_sweep", "world": self.world, "channels": self.C, "samples": self.T, "slab": self.slab, "points": summarise(gathered, self.points),
               "gather": path, "msamples_per_s": samples / times[0] / 1e6, "msamples_per_s_runs": samples / times[2] / 1e6,
               "seconds": {"loop": times[0], "synthesis": times[1], "runs": times[2]},
               "parity_vs_oracle": {"checked": int(times[3]), "mismatches": int(times[4])}}
        print(json.dumps(res), flush=True)
        return int(times[4] > 0)

    def gather(self, mine):
        """All words at rank 0 in rank (= channel) order: the library's gather over RCCL, the torch.distributed one if every rank cannot have it."""
        m17hip, dist = self.m17hip, self.dist
        if dist is None:
            return mine, "none (1 GPU)"
        import torch

        def all_ok(flag):
            t = torch.tensor([1 if flag else 0], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(t.item())

        comm = None
        try:
            cid = m17hip.comm_get_id() if self.rank == 0 else None
        except Exception as e:   # noqa: BLE001
            print(f"rank {self.rank}: C-ABI RCCL binding unavailable ({e})", file=sys.stderr)
            cid = None
        obj = [cid]
        dist.broadcast_object_list(obj, src=0)
        if obj[0] is not None:
            try:
                comm = m17hip.Comm(self.ctx, obj[0], self.rank, self.world)
            except Exception as e:   # noqa: BLE001
                print(f"rank {self.rank}: m17hip_comm_create failed ({e})", file=sys.stderr)
        if all_ok(comm is not None):
            out, _ = self.ctx.gather_sweep_stats(comm, mine, root=0, capacity=self.C if self.rank == 0 else None)
            comm.close()
            return out, "m17hip_gather_sweep_stats: counts all-gathered, words ncclSend/ncclRecv to rank 0"
        if comm is not None:
            comm.close()
        buf = torch.from_numpy(np.frombuffer(mine.tobytes(), dtype=np.uint8).copy())
        out, _ = self.mdist.gather_records(buf, mine.size, rec_bytes=m17hip.CHAN_STAT_DTYPE.itemsize)
        return np.frombuffer(out.numpy().tobytes(), dtype=m17hip.CHAN_STAT_DTYPE).copy(), "torch fallback (m17hip/dist.py gather_records, rec_bytes=32)"


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        env = dict(os.environ)   # (the ranks' environment: taken before _toolslib points M17HIP_LIB at the measurement build)
        import _toolslib
        return _toolslib.launch_ranks(__file__, args.gpus, argv, "metric", args.launch_timeout, dry_launch=args.dry_launch, base_env=env)
    return Sweep(args).run()


if __name__ == "__main__":
    sys.exit(main())
