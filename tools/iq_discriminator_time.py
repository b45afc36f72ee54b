"""The FM discriminator of m17hip_upload_iq_device against the float row copy of m17hip_upload_f32_device, same shape, same process, same context.
    python tools/iq_discriminator_time.py [channels [samples [repeats]]]        (default 4096 x 480 000, 5 timed uploads per kind)
Per kind: the kernel's own device time where the library times it (m17hip_timing_get "discriminate": events bound to the launch), the time between two
events recorded on the context's main stream around the call (the copy kernel has no timer of its own), and the wall time of the synchronous call.  The
discriminator moves 12 B (float IQ) or 8 B (int16 IQ) per sample where the copy moves 8 B; above twice the copy's time it would be compute-shaped.
The shader clock is sampled from sysfs (read only) while the uploads run."""
import glob, json, os, sys, threading, time
if not os.environ.get("GPU_MAX_HW_QUEUES", "").isdigit() or int(os.environ["GPU_MAX_HW_QUEUES"]) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"   # (before torch initialises the HIP runtime: a context's streams must not share hardware queues)
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'm17-cxx-demod_amd'))
import m17hip

C = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 480000
REP = int(sys.argv[3]) if len(sys.argv) > 3 else 5


class Clocks(threading.Thread):
    """The highest current sclk (MHz) seen per card while it runs."""
    def __init__(self):
        super().__init__(daemon=True)
        self.files = sorted(glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk'))
        self.seen, self.stop = {}, False

    def run(self):
        while not self.stop:
            for f in self.files:
                try:
                    cur = [l for l in open(f).read().splitlines() if l.rstrip().endswith('*')]
                    mhz = int(''.join(ch for ch in cur[0].split(':')[1] if ch.isdigit())) if cur else 0
                    self.seen[f.split('/')[4]] = max(self.seen.get(f.split('/')[4], 0), mhz)
                except Exception:
                    pass
            time.sleep(0.002)


ctx = m17hip.Context(C, T)
stream = ctx.torch_stream()
g = torch.Generator(device='cuda').manual_seed(608)
src = {
    "copy_f32": torch.randn((C, T), dtype=torch.float32, device='cuda', generator=g),
    "iq_i16": torch.randint(-20000, 20000, (C, T, 2), dtype=torch.int16, device='cuda', generator=g),
    "iq_f32": torch.view_as_complex(torch.randn((C, T, 2), dtype=torch.float32, device='cuda', generator=g) * 12000.0),
}
torch.cuda.synchronize()


def call(kind):
    t = src[kind]
    if kind == "copy_f32":
        ctx.upload_device(t.data_ptr(), C, T, dtype=np.float32)
    else:
        ctx.upload_iq_device(t.data_ptr(), C, T, iq_format=m17hip.IQ_I16 if kind == "iq_i16" else m17hip.IQ_F32)


out = {"channels": C, "samples": T, "repeats": REP}
clocks = Clocks()
clocks.start()
for kind in src:
    ctx.reset()
    call(kind)   # warm-up (allocations, first launch)
    ctx.timing(True); ctx.timing_reset()
    ev, wall = [], []
    for _ in range(REP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter(); call(kind); wall.append((time.perf_counter() - t0) * 1e3)
        b.record(stream)
        b.synchronize()
        ev.append(a.elapsed_time(b))
    ms, n = ctx.timing_get("discriminate")
    ctx.timing(False)
    out[kind] = {"stream_ms": [round(v, 3) for v in ev], "stream_ms_median": round(float(np.median(ev)), 3), "wall_ms_median": round(float(np.median(wall)), 3),
                 "kernel_ms": round(ms / n, 3) if n else None, "bytes_per_sample": {"copy_f32": 8, "iq_i16": 8, "iq_f32": 12}[kind]}
    out[kind]["GBps"] = round(C * T * out[kind]["bytes_per_sample"] / (out[kind]["kernel_ms"] or out[kind]["stream_ms_median"]) / 1e6, 1)
clocks.stop = True
for kind in ("iq_i16", "iq_f32"):
    out[kind]["over_copy"] = round(out[kind]["kernel_ms"] / out["copy_f32"]["stream_ms_median"], 3)
out["sclk_mhz_max_seen"] = clocks.seen
out["iq_bytes"] = ctx.iq_bytes()
print(json.dumps(out))
