"""A loopback at full scale: a TX context synthesises m17hip_synth_tx_i16 content for C channels, multiplexes it onto S wide IQ streams on the device
(m17hip_synth_wide_device: wide_tx_prefix_kernel and wide_tx_mux_kernel, csrc/m17_wide_tx_kernels.hpp), an RX context takes the streams with
m17hip_upload_wide_device under a named configuration and runs; the tool counts the channels whose good records (Viterbi cost below 30, no LICH) hold the
content sent.
    python tools/wide_loopback.py [--decim R | --decim2 R1 R2 | --raster R M | --rate HZ] [--channels C] [--sources S] [--outputs T] [--amplitude A]
                                  [--sigma SIGMA] [--spacing HZ] [--squelch DB [--points N] [--blocks K] [--hang H]]
--decim R        one-stage tuner (m17hip_wide_config) at 48000 R                      (the default: --decim 5)
--decim2 R1 R2   two-stage tuner (m17hip_wide_config2) at 48000 R1 R2                 (2.4 MSPS: --decim2 10 5)
--raster R M     polyphase channeliser (m17hip_wide_raster) at 48000 R, M bins        (2.4 MSPS, 12.5 kHz: --raster 50 192)
--rate HZ        resampling tuner (m17hip_wide_resample) at the rate's ratio          (2.048 MSPS: --rate 2048000)
Defaults: 4096 channels on 64 sources, 48 000 outputs, int16 streams.  A source's channels sit --spacing Hz apart (default 12 500; on a raster the bin
spacing) around its centre, as many as fit between +-0.45 of the rate; channels that do not fit wrap onto the same offsets again — they then share a
carrier and cannot decode, which the count shows: 64 channels of 12.5 kHz need 800 kHz.  The amplitude defaults to the largest for which
n A + 8 sigma <= 32767 with n channels on a source, so no sample clips.
With --squelch DB (a tuner, not --raster) the same streams are received once more with the spectrum squelch on (m17hip_wide_squelch): one unsquelched block's
spectrum plane (--points N, default 2048, hop N) gives the levels — m17hip.wide_squelch_levels: a 9 kHz band, open DB and close DB - 3 dB over the median
floor —, then the outputs go in --blocks K equal blocks (default 1), each a run of its own, and the channels decoded from the squelched feed are counted
beside those of the unsquelched one: the difference is what the squelch costs in lost lead-ins.
Printed, as one JSON line: the channels decoded — beside how many of the same basebands decode when the TX context demodulates its own slab, with no
multiplex in between, and how many do both ways —, the generator's time (library timer "synth_wide": both kernels) beside its instruction-count floor and the
time of a device-to-device copy of the same output bytes, and the receive kernel's time (its library timer).
The floor counts, per (channel, wideband sample), WTX_OPS plain vector operations from detail/core.h: the oscillator's 2 + 2 x 8 + 2 multiplies and adds
and 9 integer / select steps (29), wtx_within's 2 multiplies, an add and a 32 x 32 -> 64 product (5), the top half of base + K within — four 32-bit
products, three adds, an add with carry (9) —, the carrier's multiply and two adds (3), the term's two multiplies and two adds (4) and three LDS reads:
53; at 32 lane-operations per clock and SIMD (a plain wave64 instruction every 2 clocks), 4 SIMDs a CU, the highest shader clock level the driver lists."""
import ctypes as C
import glob, json, os, re, sys
if not os.environ.get("GPU_MAX_HW_QUEUES", "").isdigit() or int(os.environ["GPU_MAX_HW_QUEUES"]) < 16:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"   # (before torch initialises the HIP runtime: a context's streams must not share hardware queues)
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'm17-cxx-demod_amd'))
import m17hip

WTX_OPS = 53
BERT, STREAM, PACKET = m17hip.TX_BERT, m17hip.TX_STREAM, m17hip.TX_PACKET
FT_LSF, FT_LICH, FT_STREAM = 0, 1, 2


def take(args, flag, n, default):
    if flag not in args:
        return default
    k = args.index(flag)
    v = args[k + 1:k + 1 + n]
    del args[k:k + 1 + n]
    return v[0] if n == 1 else v


ARGS = sys.argv[1:]
DECIM2 = take(ARGS, "--decim2", 2, None)
RASTER = take(ARGS, "--raster", 2, None)
RATE = take(ARGS, "--rate", 1, None)
DECIM = take(ARGS, "--decim", 1, None)
C_ALL = int(take(ARGS, "--channels", 1, 4096))
S = int(take(ARGS, "--sources", 1, 64))
T = int(take(ARGS, "--outputs", 1, 48000))
SIGMA = float(take(ARGS, "--sigma", 1, 100.0))
AMP = take(ARGS, "--amplitude", 1, None)
SPACING = float(take(ARGS, "--spacing", 1, 12500.0))
SQUELCH = take(ARGS, "--squelch", 1, None)
POINTS = int(take(ARGS, "--points", 1, 2048))
BLOCKS = int(take(ARGS, "--blocks", 1, 1))
HANG = int(take(ARGS, "--hang", 1, 0))
assert not ARGS, f"unknown arguments {ARGS}"
assert SQUELCH is None or not RASTER, "--squelch goes with a tuner"
assert sum(v is not None for v in (DECIM2, RASTER, RATE, DECIM)) <= 1, "one configuration"
assert C_ALL % S == 0, "the same number of channels on every source"
PER = C_ALL // S

if DECIM2:
    R1, R2 = int(DECIM2[0]), int(DECIM2[1])
    P, Q, name, timer = R1 * R2, 1, f"decim2 {R1} x {R2}", "tune2"
elif RASTER:
    R, M = int(RASTER[0]), int(RASTER[1])
    P, Q, name, timer = R, 1, f"raster {R} / {M}", "channelise"
    SPACING = 48000.0 * R / M
elif RATE:
    D1, UP, DOWN = m17hip.wide_resample_ratio(int(RATE))
    P, Q, name, timer = D1 * DOWN, UP, f"rate {int(RATE)} ({D1} x {DOWN} / {UP})", "resample"
else:
    R = int(DECIM or 5)
    P, Q, name, timer = R, 1, f"decim {R}", "tune"
T = T // Q * Q
RATE_HZ = 48000.0 * P / Q
W = T // Q * P

# a source's offsets: multiples of the spacing around the centre, as many as fit; the rest wrap onto them again
fit = max(int(0.9 * RATE_HZ / SPACING), 1)
steps = [(i % fit) - fit // 2 for i in range(PER)]
hz = [SPACING * s for s in steps]
shared = PER - len(set(steps))


def content(c, rng):
    """Channel c's transmission: BERT, stream and packet in turn, four payload frames of random content."""
    kind, n = c % 3, 4
    if kind == BERT:
        return (kind, None, [bytes(rng.integers(0, 256, 24, dtype=np.uint8)) + bytes([int(rng.integers(0, 32)) << 3]) for _ in range(n)])
    if kind == STREAM:
        lsf = m17hip.make_lsf("N0CALL", "AB1CDE-9", 0x0005 | (c % 16) << 7, bytes(rng.integers(0, 256, 14, dtype=np.uint8)))
        return (kind, lsf, [m17hip.stream_row(i, rng.integers(0, 256, 16, dtype=np.uint8), last=i == n - 1) for i in range(n)])
    lsf = m17hip.make_lsf("W1AW/P", "SP5WWP", 0x0002)
    return (kind, lsf, [bytes(rng.integers(0, 256, 25, dtype=np.uint8)) + bytes([0x80 | 25 << 2 if i == n - 1 else i << 2]) for i in range(n)])


def sent(r, transmission):
    kind, lsf, rows = transmission
    r = r[(r["cost"] < 30) & (r["frame_type"] != FT_LICH)]
    n = {BERT: 25, STREAM: 18, PACKET: 26}[kind]
    pay = r[r["frame_type"] == FT_STREAM] if kind == STREAM else r[r["frame_type"] != FT_LSF]
    ok = [bytes(q["payload"][:n]) for q in pay][:len(rows)] == [bytes(row[:n]) for row in rows]
    if kind != BERT:
        ok = ok and r.size > 0 and r[0]["frame_type"] == FT_LSF and bytes(r[0]["payload"][:30]) == bytes(lsf)
    return ok


class SynthParams(C.Structure):   # m17_synth_params (include/m17hip.h)
    _fields_ = [("seed", C.c_uint64), ("kind", C.c_int32), ("n_frames", C.c_int32), ("lead_in", C.c_int32), ("phase", C.c_int32), ("tail", C.c_int32),
                ("total", C.c_int32), ("invert", C.c_int32), ("n_preamble", C.c_int32), ("lead_sigma", C.c_double), ("noise_sigma", C.c_double),
                ("dc_offset", C.c_double), ("gain", C.c_double), ("tail_sigma", C.c_double)]


rng = np.random.default_rng(617)
transmissions = [content(c, rng) for c in range(C_ALL)]
# (the loud lead-in the reference's demodulator acquires behind: tests/test_gpu_synth_tx.py)
base = SynthParams(seed=1, kind=1, n_frames=0, lead_in=3072, phase=-1, tail=0, total=0, invert=0, n_preamble=0, lead_sigma=40000.0, noise_sigma=0.0,
                   dc_offset=0.0, gain=1.0, tail_sigma=100.0)
amp = float(AMP) if AMP is not None else float(int((32767.0 - 8.0 * SIGMA) / PER))
assert PER * amp + 8.0 * SIGMA <= 32767.0, "n A + 8 sigma <= 32767: no sample may clip"
src = np.arange(C_ALL, dtype=np.uint32) // PER
fcw = [m17hip.wide_fcw(hz[c % PER], P / Q) for c in range(C_ALL)]

tx = m17hip.Context(C_ALL, T)
tx.synth_tx(base, transmissions, T)
tx.synth_wide_config(S, P, Q, m17hip.IQ_I16, None, SIGMA, 5, 0)
tx.synth_wide_channels(src, fcw, 0, amp)
out = torch.zeros((S, W, 2), dtype=torch.int16, device="cuda")
torch.cuda.synchronize()
tx.synth_wide(out=out)   # (the first block allocates the scratch plane and brings the table)
tx.reset()
tx.timing(True)
tx.timing_reset()
tx.synth_wide(out=out)
gen_ms, gen_n = tx.timing_get("synth_wide")
tx_bytes = tx.iq_bytes()
clipped = int(((out == 32767) | (out == -32768)).sum().item())
# for scale: the same basebands demodulated where they are, no multiplex in between (the TX context is a demodulation context like any other)
tx.reset()
tx.run()
direct = tx.frames()
tx.close()

a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
dup = torch.empty_like(out)
dup.copy_(out)
torch.cuda.synchronize()
a.record()
dup.copy_(out)
b.record()
torch.cuda.synchronize()
copy_ms = a.elapsed_time(b)
del dup

rx = m17hip.Context(C_ALL, T)
if DECIM2:
    rx.wide_config2(S, R1, R2)
    rx.wide_channels(src, fcw)
elif RASTER:
    rx.wide_raster(S, R, M)
    rx.wide_raster_channels(src, [m17hip.wide_bin(hz[c % PER], R, M) for c in range(C_ALL)])
elif RATE:
    rx.wide_resample(S, D1, UP, DOWN)
    rx.wide_channels(src, fcw)
else:
    rx.wide_config(S, R)
    rx.wide_channels(src, fcw)
rx.reset()
rx.timing(True)
rx.timing_reset()
rx.upload_wide_device(out.data_ptr(), C_ALL, T, W)
rx.run()
recs = rx.frames()
rx_ms, rx_n = rx.timing_get(timer)
squelched = None
if SQUELCH is not None:   # the same streams once more, squelched: levels from one unsquelched block's plane, then K blocks, each a run
    assert T % (BLOCKS * Q) == 0, "--blocks K: equal blocks of whole groups"
    Tb = T // BLOCKS
    Wb = Tb // Q * P
    half = m17hip.wide_squelch_half_bins(9000.0, RATE_HZ, POINTS)
    rx.reset()
    rx.wide_spectrum(POINTS, POINTS)
    rx.upload_wide_device(out.data_ptr(), C_ALL, T, W)
    power, frames, _ = rx.wide_spectrum_fetch()
    levels = m17hip.wide_squelch_levels(power, frames, half, float(SQUELCH), float(SQUELCH) - 3.0)
    rx.reset()
    rx.wide_squelch(half, levels[0], levels[1], HANG)
    rx.timing_reset()
    parts, opened = [], []
    for k in range(BLOCKS):
        rx.upload_wide_device(out.data_ptr() + k * Wb * 4, C_ALL, Tb, W)
        rx.run()
        parts.append(rx.frames().copy())
        opened.append(int(rx.wide_squelch_fetch()[0].sum()))
    squelched = {"margin_db": float(SQUELCH), "points": POINTS, "half_bins": half, "blocks": BLOCKS, "hang": HANG, "open_channels_per_block": opened,
                 "records": np.concatenate(parts), "tuner_ms": rx.timing_get(timer)[0] / BLOCKS, "spectrum_ms": rx.timing_get("spectrum")[0] / BLOCKS,
                 "squelch_kernel_ms": rx.timing_get("squelch")[0] / BLOCKS}
rx.close()



def failures(recs):
    recs = recs[np.argsort(recs["channel"], kind="stable")]
    cuts = np.searchsorted(recs["channel"], np.arange(C_ALL + 1))
    return [c for c in range(C_ALL) if not sent(recs[cuts[c]:cuts[c + 1]], transmissions[c])]


bad, bad_direct = failures(recs), failures(direct)
if squelched is not None:
    bad_sq = failures(squelched.pop("records"))
    squelched.update(decoded=C_ALL - len(bad_sq), decoded_unsquelched=C_ALL - len(bad), lost_to_the_squelch=len(set(bad_sq) - set(bad)),
                     first_lost=sorted(set(bad_sq) - set(bad))[:16])
cus = torch.cuda.get_device_properties(0).multi_processor_count
mhz = 2400.0   # (the highest shader clock level the driver lists, read only; 2400 where it lists none)
for path in sorted(glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk')):
    try:
        levels = [float(m.group(1)) for m in (re.search(r'(\d+)\s*[Mm][Hh]z', line) for line in open(path)) if m]
    except OSError:
        continue
    if levels:
        mhz = max(levels)
        break
floor_ms = float(C_ALL) * W * WTX_OPS / (32.0 * 4 * cus * mhz * 1e6) * 1e3
print(json.dumps({
    "configuration": name, "rate_hz": RATE_HZ, "channels": C_ALL, "sources": S, "outputs": T, "row_samples": W, "spacing_hz": SPACING,
    "channels_sharing_an_offset_per_source": shared, "amplitude": amp, "sigma": SIGMA, "clipped_samples": clipped,
    "decoded": C_ALL - len(bad), "first_failures": bad[:16],
    "decoded_from_the_basebands_directly": C_ALL - len(bad_direct), "decoded_by_both": C_ALL - len(set(bad) | set(bad_direct)),
    "generator_ms": gen_ms / max(gen_n, 1), "generator_floor_ms": floor_ms, "generator_x_floor": gen_ms / max(gen_n, 1) / floor_ms,
    "copy_same_bytes_ms": copy_ms, "output_bytes": int(out.numel() * 2), "generator_device_bytes": tx_bytes,
    "receive_kernel": timer, "receive_ms": rx_ms / max(rx_n, 1), **({"squelched": squelched} if squelched is not None else {}), "cus": cus, "shader_mhz_max_level": mhz}))
