"""The tuner of m17hip_upload_wide_device (tune_kernel, csrc/m17_wide_kernels.hpp) at a receiver's shape, against its own VALU floor.
    python tools/wide_time.py [--decim2 R2 | --resample UP DOWN | --raster M [--survey STRIDE]] [--spectrum N --hop H [--squelch FRACTION[,FRACTION...]] [--squelch-floor FRACTION[,FRACTION...]] [--scan POOL] [--slots KEYED[,KEYED...]]] [--meter W] [sources [channels_per_source [outputs [decim [repeats]]]]]     (default 64 x 64 = 4096 channels, 48 000 outputs, R = 5, 10 timed blocks)
int16 input, device form, default taps (L = 32 R + 1).  With --decim2 R2 it is the two-stage tuner of m17hip_wide_config2 (tune2_kernel,
csrc/m17_wide2_kernels.hpp; library timer "tune2") at decim x R2 with the default taps of both stages: the filter term of the floor is then
C T (R2 L1 + L2) — R2 first-stage sums of L1 taps and one second-stage sum of L2 per output — and the mixing term C T decim R2 samples.  The kernel's own device time comes from the library (m17hip_timing_get "tune": events bound to the
launch); the time between two events on the context's main stream around the call and the wall time of the synchronous call are printed beside it.
The floor counts what the algorithm needs from the shapes, at the f32 vector rate of the chip (64 FLOP per clock and SIMD: a packed fma wave instruction
— two chains of 64 outputs by one tap — every 4 clocks, a plain one every 2):
    filter:  C T L packed fma per lane, / 64 lanes
    mixing:  C T R samples (each channel mixes its own copy: independent of the number of sources), MIX_OPS plain vector operations each — counted from
             detail/core.h: the oscillator's 2 + 2 x 8 + 2 multiplies and adds and 9 integer / select steps, fm_cross's 6, 2 conversions, 3 address steps
over 4 SIMDs x CUs x the shader clock seen while the blocks ran (read from sysfs, read only).
With --raster M it is the channeliser of m17hip_wide_raster (chan_kernel, csrc/m17_chan_kernels.hpp; library timer "channelise") at `decim` (1..64) with the
default taps, every source heard on channels_per_source distinct bins.  Its floor is counted per SOURCE and output, not per channel:
    fold:    S T L packed fma (every tap meets one sample)
    pass 1:  S T M M2 complex steps of 4 plain fma, M = M1 x M2 as the library factors it
    pass 2:  C T M1 complex steps of 4 plain fma
and no mixing term: there is no oscillator.
With --survey STRIDE beside --raster the same blocks are then timed once more with the raster survey on (m17hip_wide_survey; chan_survey_kernel and
chan_survey_sum_kernel, csrc/m17_chan_survey_kernels.hpp; library timer "survey"): the channeliser's time with the survey on and the survey's own, against
the survey's floor, counted per source and SURVEY TIME (outputs / STRIDE of them): L packed fma for the fold, M M2 steps of 4 plain fma for pass 1 and
M M1 for pass 2 — all M bins.
With --resample UP DOWN it is the resampling tuner of m17hip_wide_resample (resample_kernel, csrc/m17_resample_kernels.hpp; library timer "resample") at
`decim` x DOWN / UP with the default taps of both stages (2.048 MSPS: --resample 3 8 ... 16); outputs are rounded down to a multiple of UP.  The filter term
of its floor is C T (DOWN / UP L1 + L2 / UP) packed fma — DOWN / UP first-stage sums per output and the L2 / UP taps of the second stage that meet a sample —
and the mixing term C T decim DOWN / UP samples.  In the same call the UNCHANGED tune2_kernel is then timed on the same buffer at the neighbouring integer
shape decim x round(DOWN / UP) (at UP = 1 the very same shape, where the two kernels compute the same words): "neighbour" in the result.
With --spectrum N --hop H under any of them the same blocks are then timed once more with the source spectrum on (m17hip_wide_spectrum; spectrum_kernel,
csrc/m17_spectrum_kernels.hpp, and chan_survey_sum_kernel; library timer "spectrum"): the configuration's own kernel with the spectrum on beside its time
with it off, the spectrum's own time, a device-to-device copy of the same block bytes as the memory yardstick, and the spectrum's floor — 5 N log2 N
flops per frame at the packed rate, 64 per clock and SIMD.
With --meter W under any of them the same blocks are then timed once more with the channel meter on (m17hip_wide_meter; the METERED instantiation of the
configuration's kernel, which stores chan_power of every z, and wide_meter_kernel, csrc/m17_meter_kernels.hpp; library timer "meter"): the metered kernel
beside the unmetered one of the same call, the meter kernel's own time, and a device-to-device copy of the bytes it reads — 2 x 4 bytes per channel and
output — as the memory yardstick.
With --squelch FRACTION[,FRACTION...] beside --spectrum under one of the three tuners a source of weak noise is made with a carrier on that fraction of the
channels (a random choice among every source's channels: the first ones of every source put the open workgroups at a fixed period of the grid, which was
measured 4 x slower per open workgroup under the two-stage tuners), one unsquelched block's plane gives the levels (m17hip.wide_squelch_levels: a 9 kHz band, open 10 dB and
close 6 dB over the median floor), and the squelched launch — the spectrum, wide_squelch_kernel (library timer "squelch") and the squelched instantiation of
the tuner — is timed per fraction beside the unsquelched tuner and spectrum on the same source in the same call.  Fraction 0 is a grid of all-closed
workgroups: the floor of the design.
With --squelch-floor FRACTION[,FRACTION...] the same sources are squelched (block mode, 10 / 6 dB) with the floor taken ON THE DEVICE
(m17hip_wide_squelch_floor: squelch_floor_kernel, library timer "squelch_floor", beside the spectrum's of the same call), and then at given levels equal to
the ones the device derived for the last block (where the block is no whole number of hops the frames shift from block to block, and a channel at the
margin may decide differently: both counts are reported): the two launches — spectrum + floor + squelch + tuner against spectrum + squelch + tuner —
side by side.
With --scan POOL beside --spectrum (at most 4096 points) the first POOL channels of every source are slots of the carrier scan (m17hip_wide_scan:
wide_scan_kernel, library timer "scan"), a carrier stands on a tenth of every source's channels, block mode at 10 / 6 dB with the floor on the device: the
scan kernel beside squelch_floor_kernel of the same call, and the scanned launch — spectrum + floor + scan + squelch + tuner — beside the same launch of
the same build with the scan off and the scan's fetched table given through m17hip_wide_channels, twice (the second pass is the yardstick's own spread).
With --slots KEYED[,KEYED...] beside --spectrum under one of the three tuners EVERY channel has a carrier, keyed for the first KEYED (0 to 1) of each block
over weak noise; the levels come from the plane of a block of that noise alone (10 and 6 dB over the median floor, a 9 kHz band).  Per value the same
source is timed in the same call unsquelched (tuner and spectrum), under the block squelch (m17hip_wide_squelch: spectrum, "squelch", tuner) and under the
slot squelch (m17hip_wide_squelch_slots at lead 1, hang 1: spectrum, "squelch_slots", tuner), with the share of tiles the slot mode left open.  KEYED 1 is
the slot mode's overhead against the block mode's launch; KEYED 0.2 is what it is for."""
import glob, json, os, sys, threading, time
if not os.environ.get("GPU_MAX_HW_QUEUES", "").isdigit() or int(os.environ["GPU_MAX_HW_QUEUES"]) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"   # (before torch initialises the HIP runtime: a context's streams must not share hardware queues)
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'm17-cxx-demod_amd'))
import m17hip

ARGS = sys.argv[1:]
R2 = 0   # (0: one stage)
if "--decim2" in ARGS:
    k = ARGS.index("--decim2")
    R2 = int(ARGS[k + 1])
    del ARGS[k:k + 2]
RASTER = 0   # (0: a tuner)
if "--raster" in ARGS:
    k = ARGS.index("--raster")
    RASTER = int(ARGS[k + 1])
    del ARGS[k:k + 2]
UP = DOWN = 0   # (0: integer stages)
if "--resample" in ARGS:
    k = ARGS.index("--resample")
    UP, DOWN = int(ARGS[k + 1]), int(ARGS[k + 2])
    del ARGS[k:k + 3]
    assert not R2 and not RASTER, "--resample UP DOWN goes without --decim2 and --raster"
SURVEY = 0   # (0: not timed)
if "--survey" in ARGS:
    k = ARGS.index("--survey")
    SURVEY = int(ARGS[k + 1])
    del ARGS[k:k + 2]
    assert RASTER and SURVEY >= 1, "--survey STRIDE goes with --raster M"
SPECTRUM = HOP = 0   # (0: not timed)
if "--spectrum" in ARGS:
    k = ARGS.index("--spectrum")
    SPECTRUM = int(ARGS[k + 1])
    del ARGS[k:k + 2]
    assert "--hop" in ARGS, "--spectrum N goes with --hop H"
    k = ARGS.index("--hop")
    HOP = int(ARGS[k + 1])
    del ARGS[k:k + 2]
METER = 0   # (0: not timed)
if "--meter" in ARGS:
    k = ARGS.index("--meter")
    METER = int(ARGS[k + 1])
    del ARGS[k:k + 2]
SQUELCH = []   # (empty: not timed)
PLACE = "random"
if "--squelch-first" in ARGS:   # (the carriers on the FIRST channels of every source instead: the regular placement, kept for the comparison)
    ARGS.remove("--squelch-first")
    PLACE = "first"
if "--squelch" in ARGS:
    k = ARGS.index("--squelch")
    SQUELCH = [float(v) for v in ARGS[k + 1].split(",")]
    del ARGS[k:k + 2]
    assert SPECTRUM and not RASTER and all(0.0 <= v <= 1.0 for v in SQUELCH), "--squelch FRACTION (0 to 1) goes with --spectrum N --hop H and a tuner"
FLOOR = []   # (empty: not timed)
if "--squelch-floor" in ARGS:
    k = ARGS.index("--squelch-floor")
    FLOOR = [float(v) for v in ARGS[k + 1].split(",")]
    del ARGS[k:k + 2]
    assert SPECTRUM and not RASTER and all(0.0 <= v <= 1.0 for v in FLOOR), "--squelch-floor FRACTION (0 to 1) goes with --spectrum N --hop H and a tuner"
SCAN = 0   # (0: not timed)
if "--scan" in ARGS:
    k = ARGS.index("--scan")
    SCAN = int(ARGS[k + 1])
    del ARGS[k:k + 2]
    assert SPECTRUM and SPECTRUM <= 4096 and not RASTER and SCAN >= 1, "--scan POOL (slots per source) goes with --spectrum N (at most 4096) --hop H and a tuner"
SLOTS = []   # (empty: not timed)
if "--slots" in ARGS:
    k = ARGS.index("--slots")
    SLOTS = [float(v) for v in ARGS[k + 1].split(",")]
    del ARGS[k:k + 2]
    assert SPECTRUM and not RASTER and all(0.0 <= v <= 1.0 for v in SLOTS), "--slots KEYED (0 to 1) goes with --spectrum N --hop H and a tuner"
S = int(ARGS[0]) if len(ARGS) > 0 else 64
PER = int(ARGS[1]) if len(ARGS) > 1 else 64
T = int(ARGS[2]) if len(ARGS) > 2 else 48000
R = int(ARGS[3]) if len(ARGS) > 3 else 5
REP = int(ARGS[4]) if len(ARGS) > 4 else 10
C = S * PER
L = 32 * R + 1
RATE = R * (R2 if R2 else 1)   # wideband samples per output
if R2:
    L, L2 = (t.size for t in m17hip.wide_default_taps2(R, R2))
NEIGHBOUR = 0
if UP:
    T -= T % UP
    L, L2 = (t.size for t in m17hip.wide_resample_default_taps(R, UP, DOWN))
    NEIGHBOUR = min(max(int(round(DOWN / UP)), 1), 16)   # tune2's decim2 beside it
ROW = T // UP * DOWN * R if UP else T * RATE   # wideband samples of a source row
MIX_OPS = 40
DEMOD_STEP_MS = (20.0, 23.0)   # the demodulation step of 4096 channels x 480 000 samples (README): scaled to this shape below


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
g = torch.Generator(device='cuda').manual_seed(609)
x = torch.randint(-20000, 20000, (S, max(ROW, T * R * NEIGHBOUR), 2), dtype=torch.int16, device='cuda', generator=g)
PITCH = x.shape[1]
torch.cuda.synchronize()
rng = np.random.default_rng(609)
if RASTER:
    ctx.wide_raster(S, R, RASTER, m17hip.IQ_I16)
    ctx.wide_raster_channels(np.repeat(np.arange(S), PER), np.concatenate([rng.permutation(RASTER)[:PER] - RASTER // 2 for _ in range(S)]))
elif R2:
    ctx.wide_config2(S, R, R2, m17hip.IQ_I16)
elif UP:
    ctx.wide_resample(S, R, UP, DOWN, m17hip.IQ_I16)
else:
    ctx.wide_config(S, R, m17hip.IQ_I16)
if not RASTER:
    RATIO = R * DOWN / UP if UP else RATE
    OFFSETS = rng.uniform(-24000.0 * RATIO, 24000.0 * RATIO, C)
    ctx.wide_channels(np.repeat(np.arange(S), PER), [m17hip.wide_fcw(f, RATIO) for f in OFFSETS])


def call():
    ctx.upload_wide_device(x.data_ptr(), C, T, PITCH)


clocks = Clocks()
clocks.start()
ctx.reset()
call()   # warm-up (the table's upload, first launch)
ctx.timing(True); ctx.timing_reset()
ev, wall = [], []
for _ in range(REP):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
    b.record(stream)
    b.synchronize()
    ev.append(a.elapsed_time(b))
ms, n = ctx.timing_get("channelise" if RASTER else "tune2" if R2 else "resample" if UP else "tune")
OWN = "channelise" if RASTER else "tune2" if R2 else "resample" if UP else "tune"
spectrum = {}
if SPECTRUM:   # the same blocks once more with the spectrum on: a warm-up block (table, scratch and planes), then REP timed ones; then the copy
    ctx.wide_spectrum(SPECTRUM, HOP)
    call()
    ctx.timing_reset()
    frames = 0
    for _ in range(REP):
        call()
        frames += ctx.wide_spectrum_fetch()[1]
    (ms_o, n_o), (ms_p, n_p) = ctx.timing_get(OWN), ctx.timing_get("spectrum")
    ctx.wide_spectrum(0, 0)
    y = torch.empty_like(x[:, :ROW])
    y.copy_(x[:, :ROW])
    torch.cuda.synchronize()
    cp = []
    for _ in range(REP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); y.copy_(x[:, :ROW]); b.record()
        b.synchronize()
        cp.append(a.elapsed_time(b))
    del y
    spectrum = {"points": SPECTRUM, "hop": HOP, "launches": n_p, "frames_per_block": frames / REP, "own_kernel_ms_spectrum_off": round(ms / n, 3),
                "own_kernel_ms_spectrum_on": round(ms_o / n_o, 3), "spectrum_ms": round(ms_p / n_p, 3), "copy_ms_median": round(float(np.median(cp)), 3),
                "block_bytes": S * ROW * 4}
meter = {}
if METER:   # the same blocks once more with the meter on: a warm-up block (scratch and planes), then REP timed ones; then the copy of what the meter reads
    ctx.wide_meter(METER)
    call(); call()
    ctx.timing_reset()
    pieces = 0
    for _ in range(REP):
        call()
        pieces = ctx.wide_meter_fetch()[0].shape[2]
    (ms_o, n_o), (ms_m, n_m) = ctx.timing_get(OWN), ctx.timing_get("meter")
    ctx.wide_meter(0)
    src = torch.empty((2, C, T), dtype=torch.float32, device='cuda')
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    cp = []
    for _ in range(REP):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src); b.record()
        b.synchronize()
        cp.append(a.elapsed_time(b))
    del src, dst
    meter = {"window": METER, "launches": n_m, "pieces_per_block": pieces, "own_kernel_ms_unmetered": round(ms / n, 3),
             "own_kernel_ms_metered": round(ms_o / n_o, 3), "metered_over_unmetered": round(ms_o / n_o / (ms / n), 4), "meter_ms": round(ms_m / n_m, 3),
             "copy_ms_median": round(float(np.median(cp)), 3), "bytes_read": 2 * 4 * C * T,
             "meter_over_copy": round(ms_m / n_m / float(np.median(cp)), 2)}
def carrier_source(frac):
    """(int16 [S][ROW][2] on the device, carriers per source): weak noise with 300 exp(2 pi i f n / Fs) for that share of every source's channels, chosen at
    random (at most 64 x 300 < 32767 - 200)."""
    n64 = torch.arange(ROW, dtype=torch.float64, device='cuda')
    on = int(round(frac * PER))
    xs = torch.randint(-200, 201, (S, ROW, 2), dtype=torch.int16, device='cuda', generator=g)
    for s_ in range(S):
        pick = np.sort(rng.permutation(PER)[:on]) if PLACE == "random" else np.arange(on)
        f = torch.tensor(OFFSETS[s_ * PER + pick] / (48000.0 * RATIO), dtype=torch.float64, device='cuda')
        for k0 in range(0, on, 8):
            ph = 2.0 * np.pi * torch.remainder(f[k0:k0 + 8, None] * n64[None, :], 1.0)
            xs[s_, :, 0] += torch.round(300.0 * torch.cos(ph).sum(0)).to(torch.int16)
            xs[s_, :, 1] += torch.round(300.0 * torch.sin(ph).sum(0)).to(torch.int16)
    torch.cuda.synchronize()
    return xs, on


squelch = []
if SQUELCH:   # per fraction: a source with carriers on that share of the channels; unsquelched (spectrum + tuner), then squelched (spectrum + squelch + tuner)
    half = m17hip.wide_squelch_half_bins(9000.0, 48000.0 * RATIO, SPECTRUM)   # (at most 64: a narrower band at fine bins)
    for frac in SQUELCH:
        xs, on = carrier_source(frac)

        def call_s():
            ctx.upload_wide_device(xs.data_ptr(), C, T, ROW)

        ctx.reset()
        ctx.wide_spectrum(SPECTRUM, HOP)
        call_s(); call_s()
        power, frames, _ = ctx.wide_spectrum_fetch()
        levels = m17hip.wide_squelch_levels(power, frames, half, 10.0, 6.0)
        ctx.timing_reset()
        for _ in range(REP):
            call_s()
        ctx.wide_spectrum_fetch()
        (ms_u, n_u), (ms_pu, n_pu) = ctx.timing_get(OWN), ctx.timing_get("spectrum")
        ctx.wide_squelch(half, levels[0], levels[1], 0)
        call_s(); call_s()
        ctx.timing_reset()
        for _ in range(REP):
            call_s()
        opened = int(ctx.wide_squelch_fetch()[0].sum())
        (ms_q, n_q), (ms_pq, n_pq), (ms_k, n_k) = ctx.timing_get(OWN), ctx.timing_get("spectrum"), ctx.timing_get("squelch")
        ctx.wide_squelch(0, None)
        ctx.wide_spectrum(0, 0)
        uns, sq_ = ms_u / n_u, ms_q / n_q + ms_pq / n_pq + ms_k / n_k
        squelch.append({"fraction": frac, "placement": PLACE, "carriers": on * S, "open_channels": opened, "half_bins": half, "frames_per_block": frames,
                        "unsquelched_tuner_ms": round(uns, 3), "unsquelched_spectrum_ms": round(ms_pu / n_pu, 3), "squelched_tuner_ms": round(ms_q / n_q, 3),
                        "squelched_spectrum_ms": round(ms_pq / n_pq, 3), "squelch_kernel_ms": round(ms_k / n_k, 4), "squelched_launch_ms": round(sq_, 3),
                        "squelched_launch_over_unsquelched_tuner": round(sq_ / uns, 4)})
        del xs
    ctx.reset()
floor = []
if FLOOR:   # per fraction: the squelched launch with the floor taken on the device, beside the same launch at given levels equal to the ones the device derived
    half = m17hip.wide_squelch_half_bins(9000.0, 48000.0 * RATIO, SPECTRUM)
    ro, rc = m17hip.wide_squelch_ratio(10.0), m17hip.wide_squelch_ratio(6.0)
    for frac in FLOOR:
        xs, on = carrier_source(frac)

        def call_f():
            ctx.upload_wide_device(xs.data_ptr(), C, T, ROW)

        def timed(extra):
            call_f(); call_f()
            ctx.timing_reset()
            for _ in range(REP):
                call_f()
            opened = int(ctx.wide_squelch_fetch()[0].sum())
            parts = {k: ctx.timing_get(k) for k in (OWN, "spectrum", "squelch") + extra}
            return {k: v[0] / v[1] for k, v in parts.items()}, opened

        ctx.reset()
        ctx.wide_spectrum(SPECTRUM, HOP)
        ctx.wide_squelch(half, np.ones(S, dtype=np.float32), np.ones(S, dtype=np.float32), 0)
        ctx.wide_squelch_floor(ro, rc)
        dev_ms, dev_open = timed(("squelch_floor",))
        plane, frames = ctx.wide_squelch_floor_fetch()
        ctx.wide_squelch(half, plane[2], plane[3], 0)   # (the same block again and again: the same levels up to the frames' shift from block to block)
        giv_ms, giv_open = timed(())
        ctx.wide_squelch(0, None)
        ctx.wide_spectrum(0, 0)
        dev, giv = sum(dev_ms.values()), sum(giv_ms.values())
        floor.append({"fraction": frac, "carriers": on * S, "open_channels": dev_open, "open_channels_given_levels": giv_open, "half_bins": half, "frames_per_block": frames,
                      "floor_kernel_ms": round(dev_ms["squelch_floor"], 4), "spectrum_ms": round(dev_ms["spectrum"], 3),
                      "floor_over_spectrum": round(dev_ms["squelch_floor"] / dev_ms["spectrum"], 4), "tuner_ms_floor_on": round(dev_ms[OWN], 3),
                      "tuner_ms_given_levels": round(giv_ms[OWN], 3), "launch_ms_floor_on": round(dev, 3), "launch_ms_given_levels": round(giv, 3),
                      "floor_on_over_given": round(dev / giv, 4)})
        del xs
    ctx.reset()
scan = []
if SCAN:   # the scanned launch beside the same launch with the scan's own table given by the host
    half = m17hip.wide_squelch_half_bins(9000.0, 48000.0 * RATIO, SPECTRUM)
    guard = m17hip.wide_scan_guard_bins(9000.0, 48000.0 * RATIO, SPECTRUM)
    ro, rc = m17hip.wide_squelch_ratio(10.0), m17hip.wide_squelch_ratio(6.0)
    srcs, words0 = np.repeat(np.arange(S), PER), [m17hip.wide_fcw(f, RATIO) for f in OFFSETS]
    pool = (np.arange(C) % PER < min(SCAN, PER)).astype(np.uint8)
    xs, on = carrier_source(0.1)

    def call_c():
        ctx.upload_wide_device(xs.data_ptr(), C, T, ROW)

    def timed_c(extra):
        call_c(); call_c()
        ctx.timing_reset()
        for _ in range(REP):
            call_c()
        opened = int(ctx.wide_squelch_fetch()[0].sum())
        parts = {k: ctx.timing_get(k) for k in (OWN, "spectrum", "squelch", "squelch_floor") + extra}
        return {k: v[0] / v[1] for k, v in parts.items()}, opened

    def setup():
        ctx.reset()
        ctx.wide_spectrum(SPECTRUM, HOP)
        ctx.wide_squelch(half, np.ones(S, dtype=np.float32), np.ones(S, dtype=np.float32), 0)
        ctx.wide_squelch_floor(ro, rc)

    setup()
    ctx.wide_scan(pool, guard)
    call_c()
    first = ctx.wide_scan_fetch()
    on_ms, on_open = timed_c(("scan",))
    words, flags, missed, _ = ctx.wide_scan_fetch()
    given = []
    for _ in range(2):
        setup()
        ctx.wide_channels(srcs, words)
        given.append(timed_c(()))
    ctx.wide_channels(srcs, words0)
    ctx.wide_squelch(0, None)
    ctx.wide_spectrum(0, 0)
    tot, giv = sum(on_ms.values()), [sum(g_[0].values()) for g_ in given]
    scan.append({"slots_per_source": int(min(SCAN, PER)), "guard_bins": guard, "half_bins": half, "carriers": on * S, "assigned_first_block": len(first[3]),
                 "held_slots": int((flags & m17hip.SCAN_HELD != 0).sum()), "missed": int(missed.sum()), "open_channels": on_open,
                 "open_channels_given_table": [g_[1] for g_ in given], "scan_kernel_ms": round(on_ms["scan"], 4),
                 "floor_kernel_ms": round(on_ms["squelch_floor"], 4), "scan_over_floor": round(on_ms["scan"] / on_ms["squelch_floor"], 2),
                 "spectrum_ms": round(on_ms["spectrum"], 3), "tuner_ms_scan_on": round(on_ms[OWN], 3), "tuner_ms_given_table": [round(g_[0][OWN], 3) for g_ in given],
                 "launch_ms_scan_on": round(tot, 3), "launch_ms_given_table": [round(v, 3) for v in giv], "scan_on_over_given": round(tot / giv[0], 4),
                 "given_spread": round(giv[1] / giv[0], 4)})
    del xs
    ctx.reset()
slots = []
if SLOTS:   # per keyed share: unsquelched, block squelch, slot squelch on one source whose every channel has a carrier for the first part of each block
    assert PER * 300 + 200 <= 32767, "--slots: at most 108 channels per source (300 per carrier)"
    half = m17hip.wide_squelch_half_bins(9000.0, 48000.0 * RATIO, SPECTRUM)
    n64 = torch.arange(ROW, dtype=torch.float64, device='cuda')
    quiet = torch.randint(-200, 201, (S, ROW, 2), dtype=torch.int16, device='cuda', generator=g)
    torch.cuda.synchronize()
    ctx.reset()
    ctx.wide_spectrum(SPECTRUM, HOP)
    ctx.upload_wide_device(quiet.data_ptr(), C, T, ROW)
    power, frames, _ = ctx.wide_spectrum_fetch()
    levels = m17hip.wide_squelch_levels(power, frames, half, 10.0, 6.0)
    del quiet
    for keyed in SLOTS:
        on = int(round(keyed * ROW))
        xs = torch.randint(-200, 201, (S, ROW, 2), dtype=torch.int16, device='cuda', generator=g)
        for s_ in range(S):   # 300 exp(2 pi i f n / Fs) for every channel of the source over the block's first `on` samples
            f = torch.tensor(OFFSETS[s_ * PER:(s_ + 1) * PER] / (48000.0 * RATIO), dtype=torch.float64, device='cuda')
            for k0 in range(0, PER if on else 0, 8):
                ph = 2.0 * np.pi * torch.remainder(f[k0:k0 + 8, None] * n64[None, :on], 1.0)
                xs[s_, :on, 0] += torch.round(300.0 * torch.cos(ph).sum(0)).to(torch.int16)
                xs[s_, :on, 1] += torch.round(300.0 * torch.sin(ph).sum(0)).to(torch.int16)
        torch.cuda.synchronize()

        def timed(extra):
            ctx.upload_wide_device(xs.data_ptr(), C, T, ROW); ctx.upload_wide_device(xs.data_ptr(), C, T, ROW)
            ctx.timing_reset()
            for _ in range(REP):
                ctx.upload_wide_device(xs.data_ptr(), C, T, ROW)
            ctx.wide_spectrum_fetch()
            return sum(ctx.timing_get(name)[0] / max(ctx.timing_get(name)[1], 1) for name in (OWN, "spectrum") + extra), ctx.timing_get(OWN)[0] / REP

        ctx.reset()
        ctx.wide_spectrum(SPECTRUM, HOP)
        uns, uns_tuner = timed(())
        ctx.wide_squelch(half, levels[0], levels[1], 0)
        blk, blk_tuner = timed(("squelch",))
        blk_open = int(ctx.wide_squelch_fetch()[0].sum())
        ctx.wide_squelch_slots(half, levels[0], levels[1], 1, 1)
        slt, slt_tuner = timed(("squelch_slots",))
        state, bands, mask, tiles, frames = ctx.wide_squelch_slots_fetch()
        open_tiles = int(sum(bin(int(w)).count("1") for w in mask.reshape(-1)))
        kern = ctx.timing_get("squelch_slots")
        ctx.wide_squelch(0, None)
        ctx.wide_spectrum(0, 0)
        slots.append({"keyed": keyed, "half_bins": half, "frames_per_block": frames, "slots_per_block": int(bands.shape[1]), "tiles_per_channel": tiles,
                      "open_tile_share": round(open_tiles / float(tiles * C), 4), "block_mode_open_channels": blk_open,
                      "unsquelched_tuner_ms": round(uns_tuner, 3), "unsquelched_tuner_and_spectrum_ms": round(uns, 3),
                      "block_squelch_launch_ms": round(blk, 3), "block_squelch_tuner_ms": round(blk_tuner, 3),
                      "slot_squelch_launch_ms": round(slt, 3), "slot_squelch_tuner_ms": round(slt_tuner, 3),
                      "slot_kernels_ms": round(kern[0] / max(kern[1], 1), 4), "slot_over_block_launch": round(slt / blk, 4)})
        del xs
    ctx.reset()
neighbour = {}
if UP:   # tune2_kernel on the same buffer and table at decim x NEIGHBOUR: a warm-up block, then REP timed ones
    ctx.wide_config2(S, R, NEIGHBOUR, m17hip.IQ_I16)
    ctx.reset()
    call()
    ctx.timing_reset()
    for _ in range(REP):
        call()
    ms2, n2 = ctx.timing_get("tune2")
    l1n, l2n = (t.size for t in m17hip.wide_default_taps2(R, NEIGHBOUR))
    neighbour = {"decim2": NEIGHBOUR, "taps": l1n, "taps2": l2n, "launches": n2, "kernel_ms": round(ms2 / n2, 3),
                 "cycles": C * T * (NEIGHBOUR * l1n + l2n) / 64 * 4 + C * T * R * NEIGHBOUR * MIX_OPS / 64 * 2}
survey = {}
if SURVEY:   # the same blocks once more with the survey on: a warm-up block (the scratch and the planes are allocated), then REP timed ones
    ctx.wide_survey(SURVEY)
    call()
    ctx.timing_reset()
    times = 0
    for _ in range(REP):
        call()
        times += ctx.wide_survey_fetch()[1]
    (ms_c, n_c), (ms_s, n_s) = ctx.timing_get("channelise"), ctx.timing_get("survey")
    survey = {"stride": SURVEY, "launches": n_s, "times_per_block": times / REP, "channelise_ms_survey_on": round(ms_c / n_c, 3), "survey_ms": round(ms_s / n_s, 3)}
ctx.timing(False)
clocks.stop = True
cus = torch.cuda.get_device_properties(0).multi_processor_count
mhz = max(clocks.seen.values()) if clocks.seen else 2400
FILTER = C * T * (R2 * L + L2 if R2 else L) / 64 * 4
cycles = FILTER + C * T * RATE * MIX_OPS / 64 * 2
if UP:
    FILTER = C * T * (DOWN / UP * L + L2 / UP) / 64 * 4
    cycles = FILTER + C * T * R * DOWN / UP * MIX_OPS / 64 * 2
if RASTER:
    M2 = max(d for d in range(1, RASTER + 1) if RASTER % d == 0 and d * d <= RASTER)
    M1 = RASTER // M2
    FILTER = S * T * L / 64 * 4
    cycles = FILTER + (S * T * RASTER * M2 + C * T * M1) * 4 / 64 * 2
floor_ms = cycles / (4 * cus * mhz * 1e6) * 1e3
if SURVEY:
    sc = S * survey["times_per_block"] * (L / 64 * 4 + (RASTER * M2 + RASTER * M1) * 4 / 64 * 2)
    survey["floor_ms"] = round(sc / (4 * cus * mhz * 1e6) * 1e3, 4)
    survey["survey_over_floor"] = round(survey["survey_ms"] / (sc / (4 * cus * mhz * 1e6) * 1e3), 2)
if SPECTRUM:
    pc = S * spectrum["frames_per_block"] * 5 * SPECTRUM * (SPECTRUM.bit_length() - 1) / 64
    pf = pc / (4 * cus * mhz * 1e6) * 1e3
    spectrum.update(floor_ms=round(pf, 4), spectrum_over_floor=round(spectrum["spectrum_ms"] / pf, 2) if pf else None,
                    spectrum_over_copy=round(spectrum["spectrum_ms"] / spectrum["copy_ms_median"], 2))
kernel_ms = ms / n
if UP:
    nf = neighbour.pop("cycles") / (4 * cus * mhz * 1e6) * 1e3
    neighbour.update(floor_ms=round(nf, 3), kernel_over_floor=round(neighbour["kernel_ms"] / nf, 2), resample_over_tune2=round(kernel_ms / neighbour["kernel_ms"], 3))
step = [v * T / 480000.0 * C / 4096.0 for v in DEMOD_STEP_MS]
print(json.dumps({
    "sources": S, "channels": C, "outputs": T, "decim": R, "taps": L, **({"decim2": R2, "taps2": L2} if R2 else {}),
    **({"raster": RASTER} if RASTER else {}), **({"up": UP, "down": DOWN, "taps2": L2, "neighbour": neighbour} if UP else {}), "repeats": REP, "launches": n,
    "kernel_ms": round(kernel_ms, 3), "stream_ms": [round(v, 3) for v in ev], "stream_ms_median": round(float(np.median(ev)), 3),
    "wall_ms_median": round(float(np.median(wall)), 3),
    "floor_ms": round(floor_ms, 3), "floor_filter_share": round(FILTER / cycles, 3), "kernel_over_floor": round(kernel_ms / floor_ms, 2),
    "demod_step_ms_same_samples": [round(v, 3) for v in step], "tuner_over_demod_step": [round(kernel_ms / v, 2) for v in step],
    **({"survey": survey} if SURVEY else {}), **({"spectrum": spectrum} if SPECTRUM else {}), **({"meter": meter} if METER else {}), **({"squelch": squelch} if SQUELCH else {}), **({"squelch_floor": floor} if FLOOR else {}), **({"scan": scan} if SCAN else {}), **({"slots": slots} if SLOTS else {}),
    "cus": cus, "sclk_mhz_max_seen": clocks.seen, "iq_bytes": ctx.iq_bytes(),
}))
