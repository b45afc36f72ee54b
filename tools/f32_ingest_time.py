"""One step on the float path against the same signal as int16, in one process and one context: per-kernel device time (m17hip_timing_*) and wall time.
    python tools/f32_ingest_time.py [channels [samples [repeats]]]        (default 4096 x 480 000, 3 timed steps per format)
The signal is synthesised on the device as int16 (the bench workload), read back, and uploaded again as float(s / 41067.0): the two passes decode the
same frames (asserted), so the difference is the input format alone — 4 instead of 2 input bytes per sample and the float forms of K1, K3, K2, K5."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'm17-cxx-demod_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import m17hip, oracle_lib as ol

C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 480000
REP = int(sys.argv[3]) if len(sys.argv) > 3 else 3
KERNELS = ("fir_rrc150", "dcd", "limit_track", "demod_seq", "decode")

p = ol.gen_params(seed=20260101, kind=-1, n_frames=T // 1920 - 6, lead_in=3072, noise_sigma=600., tail_sigma=600., lead_sigma=40000.0, total=T)
ctx = m17hip.Context(C, T)
ctx.synth(p, C, T)
s = ctx.download()
x = np.empty((C, T), dtype=np.float32)
for c0 in range(0, C, 64):   # (row blocks: the double intermediate of the whole slab would be 8 bytes per sample)
    x[c0:c0 + 64] = (s[c0:c0 + 64].astype(np.float64) / 41067.0).astype(np.float32)


def one_format(data):
    ctx.reset()          # frees the stream's format
    ctx.upload(data)
    ctx.reset(); ctx.run(); n_frames = ctx.frames_count()   # warm-up (allocations, first launches)
    ctx.timing(True); ctx.timing_reset()
    wall = []
    for _ in range(REP):
        ctx.reset()
        t0 = time.perf_counter(); ctx.run(); assert ctx.frames_count() == n_frames; wall.append((time.perf_counter() - t0) * 1e3)
    per = {k: round(ctx.timing_get(k)[0] / REP, 3) for k in KERNELS}
    ctx.timing(False)
    return {"wall_ms": [round(w, 2) for w in wall], "wall_ms_median": round(float(np.median(wall)), 2), "kernel_ms_per_step": per, "frames": int(n_frames)}


out = {"channels": C, "samples": T, "repeats": REP, "int16": one_format(s), "float32": one_format(x)}
assert out["int16"]["frames"] == out["float32"]["frames"], "the two formats must decode the same frames"
out["float_over_int16_wall"] = round(out["float32"]["wall_ms_median"] / out["int16"]["wall_ms_median"], 4)
out["f32_bytes"] = ctx.input_format()[1]
print(json.dumps(out))
