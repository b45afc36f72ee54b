"""Python (ctypes) binding of the C ABI in include/m17hip.h — the MI355X-native M17 demodulation hot path.

This is plumbing over `libm17hip.so` (hand-written HIP kernels for gfx950): no CPU fallback exists and
none is attempted — if the library is missing or a HIP call fails, a `M17HipError` is raised.
Nothing here imports the oracle.
"""
import ctypes as C
import os

import numpy as np

# The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises (a context's five streams must not share hardware queues: include/m17hip.h,
# m17hip_advice): ask for 16 unless the host has decided otherwise.  Effective when this import comes before the process's first contact with
# the GPU; m17hip_ctx_create refuses (M17HIP_ECONFIG) when fewer than 8 were asked for.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M17HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libm17hip.so")   # (M17HIP_LIB: an experiment build of the same library)

FRAME_REC = np.dtype(
    [("channel", "<u4"), ("seq", "<u4"), ("sample_pos", "<u8"), ("cost", "<i4"), ("frame_type", "u1"), ("sync_type", "u1"),
     ("len", "u1"), ("flags", "u1"), ("payload", "u1", (32,)), ("pad", "u1", (8,))]
)
DIAG = np.dtype(
    [("dcd", "<i4"), ("evm", "<f4"), ("deviation", "<f4"), ("offset", "<f4"), ("locked", "<i4"), ("clock", "<f4"),
     ("sample_index", "<i4"), ("sync_index", "<i4"), ("clock_index", "<i4"), ("viterbi_cost", "<i4"), ("dcd_level", "<f4"),
     ("n_diag", "<u4"), ("demod_state", "<u4"), ("n_frames", "<u4"), ("pad", "<u4", (2,))]
)
assert FRAME_REC.itemsize == 64 and DIAG.itemsize == 64

FLAG_INVERT = 1
KERNELS = {"fir_rrc150": 0, "dcd": 1, "demod_seq": 2, "decode": 3, "correlator": 4, "compact": 5, "limit_track": 6, "voice": 7, "discriminate": 8, "tune": 9,
           "tune2": 10, "channelise": 11, "survey": 12, "resample": 13, "spectrum": 14, "synth_wide": 15, "meter": 16, "squelch": 17,
           "squelch_slots": 18, "squelch_floor": 19, "scan": 20}
LSF_INFO = np.dtype([("dst", "S10"), ("src", "S10"), ("type", "<u2"), ("crc_ok", "u1"), ("reserved", "u1", (9,))])
BERT_STAT = np.dtype([("bits", "<u4"), ("errors", "<u4"), ("synced", "<u4"), ("frames", "<u4")])
PACKET_REC = np.dtype([("channel", "<u4"), ("seq", "<u4"), ("sample_pos", "<u8"), ("size", "<u2"), ("checksum", "<u2"), ("crc_ok", "u1"),
                       ("frames", "u1"), ("seq_errors", "u1"), ("reserved", "u1"), ("data", "u1", (840,))])
assert PACKET_REC.itemsize == 864
CALL_REC = np.dtype([("channel", "<u4"), ("seq", "<u4"), ("start_pos", "<u8"), ("end_pos", "<u8"), ("cost_sum", "<u4"), ("frames", "<u4"),
                     ("blanked", "<u4"), ("lost", "<u4"), ("has_lsf", "u1"), ("close", "u1"), ("lsf", "u1", (30,))])   # m17_call_rec
assert CALL_REC.itemsize == 72
MARK_BLANK, MARK_EOS, MARK_FIRST, MARK_GAP = 1, 2, 4, 8   # mark bits of a voice slot (M17HIP_MARK_*)
CALL_CLOSE_EOS, CALL_CLOSE_LSF = 1, 2


def calls_per_channel(room):
    """M17HIP_CALLS_PER_CHANNEL: call records of room per channel and run for a voice room of `room` slots."""
    return int(room) // 8 + 2

VITERBI_SHAPES = {0: (488, 240), 1: (296, 144), 2: (420, 206), 3: (402, 197)}
IMPAIRMENT_DTYPE = np.dtype([("noise_sigma", "<f8"), ("tail_sigma", "<f8"), ("dc_offset", "<f8"), ("gain", "<f8")])   # m17_impairment
CHAN_STAT_DTYPE = np.dtype([("channel", "<u4"), ("point", "<u4"), ("bits", "<u4"), ("errors", "<u4"), ("synced", "<u4"), ("frames", "<u4"),
                            ("evm", "<f4"), ("flags", "<u4")])   # m17_chan_stat; flags bit 0: evm is valid
assert IMPAIRMENT_DTYPE.itemsize == 32 and CHAN_STAT_DTYPE.itemsize == 32
MAX_SWEEP_POINTS = 4096
TX_DTYPE = np.dtype([("kind", "<u4"), ("n_frames", "<u4"), ("first_row", "<u4"), ("reserved", "<u4")])   # m17_tx
WIDE_TX_DTYPE = np.dtype([("source", "<u4"), ("fcw", "<i4"), ("phase0", "<u4"), ("amplitude", "<f4")])   # m17_wide_tx
TX_BERT, TX_STREAM, TX_PACKET = 0, 1, 2

EXPORTS = [
    "m17hip_strerror", "m17hip_last_hip_error", "m17hip_version", "m17hip_ctx_create", "m17hip_ctx_destroy", "m17hip_set_stream", "m17hip_get_stream",
    "m17hip_upload_i16", "m17hip_upload_i16_device", "m17hip_upload_i16_async", "m17hip_synth_i16", "m17hip_download_i16", "m17hip_fir_rrc150", "m17hip_correlator", "m17hip_fir_correlator", "m17hip_dcd", "m17hip_viterbi",
    "m17hip_slice_llr", "m17hip_decode_frames", "m17hip_demod_reset", "m17hip_demod_run", "m17hip_frames_count", "m17hip_frames_fetch",
    "m17hip_frames_compact_device", "m17hip_diag_fetch", "m17hip_bert_stats", "m17hip_packets_fetch", "m17hip_packets_feed", "m17hip_lsf_info", "m17hip_tune", "m17hip_debug_counters", "m17hip_timing_enable", "m17hip_timing_get", "m17hip_timing_reset",
    "m17hip_set_kalman_order", "m17hip_kalman_trace", "m17hip_set_channel_base", "m17hip_upload_wait", "m17hip_comm_get_id", "m17hip_comm_create",
    "m17hip_comm_destroy", "m17hip_comm_last_error", "m17hip_gather_frames", "m17hip_gather_frames_device", "m17hip_diag_log_fetch",
    "m17hip_upload_i16_device_async", "m17hip_input_alternate", "m17hip_demod_front", "m17hip_advice", "m17hip_replay_drops", "m17hip_frames_select",
    "m17hip_synth_sweep_i16", "m17hip_sweep_stats", "m17hip_gather_sweep_stats", "m17hip_demod_reset_channels",
    "m17hip_set_channel_polarity", "m17hip_synth_tx_i16",
    "m17hip_voice_fetch", "m17hip_voice_device", "m17hip_calls_fetch", "m17hip_voice_feed",
    "m17hip_upload_f32", "m17hip_upload_f32_device", "m17hip_upload_f32_async", "m17hip_upload_f32_device_async", "m17hip_download_f32",
    "m17hip_input_format",
    "m17hip_upload_iq", "m17hip_upload_iq_device", "m17hip_upload_iq_async", "m17hip_upload_iq_device_async", "m17hip_iq_bytes",
    "m17hip_wide_default_taps", "m17hip_wide_config", "m17hip_wide_channels",
    "m17hip_upload_wide", "m17hip_upload_wide_device", "m17hip_upload_wide_async", "m17hip_upload_wide_device_async",
    "m17hip_wide_default_taps2", "m17hip_wide_config2",
    "m17hip_wide_raster_default_taps", "m17hip_wide_raster_twiddles", "m17hip_wide_raster", "m17hip_wide_raster_channels",
    "m17hip_wide_survey", "m17hip_wide_survey_fetch",
    "m17hip_wide_resample_default_taps", "m17hip_wide_resample_ratio", "m17hip_wide_resample",
    "m17hip_wide_spectrum", "m17hip_wide_spectrum_default_window", "m17hip_wide_spectrum_twiddles", "m17hip_wide_spectrum_fetch",
    "m17hip_wide_meter", "m17hip_wide_meter_shape", "m17hip_wide_meter_fetch",
    "m17hip_wide_squelch", "m17hip_wide_squelch_fetch", "m17hip_wide_squelch_slots", "m17hip_wide_squelch_slots_fetch",
    "m17hip_wide_squelch_floor", "m17hip_wide_squelch_floor_fetch", "m17hip_wide_scan", "m17hip_wide_scan_fetch",
    "m17hip_synth_wide_k", "m17hip_synth_wide_config", "m17hip_synth_wide_channels", "m17hip_synth_wide", "m17hip_synth_wide_device",
    "m17hip_decode_sequences", "m17hip_set_fir_taps",
]
FORMAT_I16, FORMAT_F32 = 1, 2   # M17HIP_FORMAT_*
IQ_I16, IQ_F32 = 1, 2           # M17HIP_IQ_*
IQ_U8 = 3                       # (wideband input only)
ETRUNC = -6
EOVERFLOW = -5
COMM_ID_BYTES = 128


class M17HipError(RuntimeError):
    pass


# ---- content of a caller-supplied transmission (Context.synth_tx), pure Python ------------------------------------------------------------
_CALLSIGN_ALPHABET = " ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-/."


def encode_callsign(call):
    """Up to 9 characters of A-Z 0-9 - / . as the 6-byte big-endian base-40 address of LinkSetupFrame.h:46-86 (first character least
    significant; any other character counts as a blank)."""
    enc = 0
    for ch in reversed(call[:9]):
        enc = enc * 40 + max(_CALLSIGN_ALPHABET.find(ch), 0)
    return enc.to_bytes(6, "big")


def crc16_m17(data):
    """CRC16<0x5935, 0xFFFF> of CRC16.h:12-70 over `data`."""
    reg = 0xFFFF
    for byte in bytes(data):
        reg ^= byte << 8
        for _ in range(8):
            reg = ((reg << 1) ^ 0x5935 if reg & 0x8000 else reg << 1) & 0xFFFF
    return reg


def make_lsf(dst, src, type_field, meta=b""):
    """The 30 bytes of a link setup frame as apps/m17-mod.cpp:310-347 fills them: destination (base 40; "" = the broadcast address FF x 6) and
    source callsigns, the 16-bit type field, up to 14 bytes of META (zero padded) and the CRC-16 over the first 28 bytes, big-endian."""
    meta = bytes(meta)
    if len(meta) > 14:
        raise ValueError("META is 14 bytes at the most")
    body = (encode_callsign(dst) if dst != "" else b"\xff" * 6) + encode_callsign(src) + int(type_field & 0xFFFF).to_bytes(2, "big") + meta.ljust(14, b"\0")
    return body + crc16_m17(body).to_bytes(2, "big")


def stream_row(fn, payload16, last=False):
    """The 32-byte row of one stream frame (apps/m17-mod.cpp:407-440): the 15-bit frame number with the end-of-stream bit, then 16 payload
    bytes; the rest is padding."""
    payload16 = bytes(payload16)
    if len(payload16) != 16:
        raise ValueError("a stream frame carries 16 payload bytes")
    return (((fn & 0x7FFF) | (0x8000 if last else 0)).to_bytes(2, "big") + payload16).ljust(32, b"\0")


_lib = None


def load_library():
    """Load libm17hip.so (built by `__graft_entry__.build()` / csrc/Makefile).  Raises if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise M17HipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                              "there is no CPU fallback for the demodulation hot path")
        lib = C.CDLL(LIB_PATH)
        lib.m17hip_strerror.restype = C.c_char_p
        lib.m17hip_comm_destroy.restype = None
        lib.m17hip_ctx_destroy.restype = None
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def wide_default_taps(decim):
    """The default low-pass of wide_config for decimation `decim`: float32 [32 * decim + 1] — m17hip_wide_default_taps (no context, no GPU)."""
    n = C.c_uint32(0)
    taps = np.zeros(32 * 16 + 1, dtype=np.float32)
    code = load_library().m17hip_wide_default_taps(C.c_uint32(decim), _ptr(taps), C.c_uint32(taps.size), C.byref(n))
    if code != 0:
        raise M17HipError(f"m17hip_wide_default_taps: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return taps[: n.value].copy()


def wide_default_taps2(decim1, decim2):
    """The default taps of wide_config2's two stages: (float32 [8 * decim1 + 1] — [1] at decim1 = 1 —, float32 [32 * decim2 + 1]) —
    m17hip_wide_default_taps2 (no context, no GPU)."""
    n1, n2 = C.c_uint32(0), C.c_uint32(0)
    t1, t2 = np.zeros(8 * 16 + 1, dtype=np.float32), np.zeros(32 * 16 + 1, dtype=np.float32)
    code = load_library().m17hip_wide_default_taps2(C.c_uint32(decim1), C.c_uint32(decim2), _ptr(t1), C.c_uint32(t1.size), C.byref(n1), _ptr(t2),
                                                    C.c_uint32(t2.size), C.byref(n2))
    if code != 0:
        raise M17HipError(f"m17hip_wide_default_taps2: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return t1[: n1.value].copy(), t2[: n2.value].copy()


def wide_raster_default_taps(decim):
    """The default low-pass of wide_raster for decimation `decim` (1..64): float32 [32 * decim + 1], wide_default_taps(decim) word for word where that
    exists — m17hip_wide_raster_default_taps (no context, no GPU)."""
    n = C.c_uint32(0)
    taps = np.zeros(32 * 64 + 1, dtype=np.float32)
    code = load_library().m17hip_wide_raster_default_taps(C.c_uint32(decim), _ptr(taps), C.c_uint32(taps.size), C.byref(n))
    if code != 0:
        raise M17HipError(f"m17hip_wide_raster_default_taps: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return taps[: n.value].copy()


def wide_resample_default_taps(decim1, up, down):
    """The default taps of wide_resample's two stages: (float32 [8 * decim1 + 1] — [1] at decim1 = 1 —, float32 [32 * down + 1] of DC gain `up`; at
    up = 1 wide_raster_default_taps(down) word for word) — m17hip_wide_resample_default_taps (no context, no GPU)."""
    n1, n2 = C.c_uint32(0), C.c_uint32(0)
    t1, t2 = np.zeros(8 * 16 + 1, dtype=np.float32), np.zeros(32 * 125 + 1, dtype=np.float32)
    code = load_library().m17hip_wide_resample_default_taps(C.c_uint32(decim1), C.c_uint32(up), C.c_uint32(down), _ptr(t1), C.c_uint32(t1.size),
                                                            C.byref(n1), _ptr(t2), C.c_uint32(t2.size), C.byref(n2))
    if code != 0:
        raise M17HipError(f"m17hip_wide_resample_default_taps: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return t1[: n1.value].copy(), t2[: n2.value].copy()


def wide_resample_ratio(rate_hz):
    """(decim1, up, down) of wide_resample for a source of `rate_hz` samples per second: rate_hz = 48000 * decim1 * down / up —
    m17hip_wide_resample_ratio (no context, no GPU).  Raises M17HipError for a rate no accepted configuration has."""
    rate = int(rate_hz)
    d1, up, down = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    code = load_library().m17hip_wide_resample_ratio(C.c_uint32(rate), C.byref(d1), C.byref(up), C.byref(down)) if 0 < rate < (1 << 32) else -1
    if code != 0:
        raise M17HipError(f"m17hip_wide_resample_ratio: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return d1.value, up.value, down.value


def wide_raster_twiddles(bins):
    """The channeliser's twiddle table for a raster of `bins`: complex64 [bins], exp(-2 pi j k / bins) made in double and rounded — the very words the
    device computes with; m17hip_wide_raster_twiddles (no context, no GPU)."""
    tw = np.zeros(max(int(bins), 1), dtype=np.complex64)
    code = load_library().m17hip_wide_raster_twiddles(C.c_uint32(bins), tw.ctypes.data_as(C.c_void_p), C.c_uint32(2 * tw.size))
    if code != 0:
        raise M17HipError(f"m17hip_wide_raster_twiddles: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return tw


def wide_bin(hz, decim, bins):
    """The bin of an offset in Hz from the source's centre on a raster of `bins` channels at 48000 * decim samples per second (wide_raster_channels).
    Raises ValueError when `hz` is not on the raster or outside it."""
    b = float(hz) * int(bins) / (48000.0 * int(decim))
    k = int(round(b))
    if abs(b - k) > 1e-9 * max(1.0, abs(b)) or k < -(int(bins) // 2) or k > (int(bins) - 1) // 2:
        raise ValueError(f"{hz} Hz is not a channel of a raster of {bins} at {48000 * int(decim)} samples per second")
    return k


def wide_raster_occupied(power, margin_db):
    """The occupied bins of a survey plane (Context.wide_survey_fetch): per source the floor is the MEDIAN of its row, and every bin more than `margin_db`
    dB above it is reported as (source, signed bin in [-M / 2, M / 2), dB over the floor), strongest first.  A row whose median is 0 or not finite reports
    nothing.  Pure numpy."""
    p = np.asarray(power, dtype=np.float32)
    if p.ndim == 1:
        p = p[None, :]
    M = p.shape[1]
    out = []
    for s in range(p.shape[0]):
        floor = float(np.median(p[s].astype(np.float64)))
        if not np.isfinite(floor) or floor <= 0.0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            db = 10.0 * np.log10(p[s].astype(np.float64) / floor)
        for k in np.nonzero(db > float(margin_db))[0]:
            out.append((s, int(k) if k <= (M - 1) // 2 else int(k) - M, float(db[k])))
    out.sort(key=lambda e: -e[2])
    return out


def wide_spectrum_default_window(points):
    """The default window of Context.wide_spectrum: float32 [points], the periodic four-term Blackman-Harris window made in double and rounded —
    m17hip_wide_spectrum_default_window (no context, no GPU)."""
    w = np.zeros(max(int(points), 1), dtype=np.float32)
    code = load_library().m17hip_wide_spectrum_default_window(C.c_uint32(points), _ptr(w), C.c_uint32(w.size))
    if code != 0:
        raise M17HipError(f"m17hip_wide_spectrum_default_window: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return w


def wide_spectrum_twiddles(points):
    """The spectrum's twiddle table: complex64 [points / 2], exp(-2 pi j k / points) made in double and rounded — the very words the device computes with;
    m17hip_wide_spectrum_twiddles (no context, no GPU)."""
    tw = np.zeros(max(int(points) // 2, 1), dtype=np.complex64)
    code = load_library().m17hip_wide_spectrum_twiddles(C.c_uint32(points), tw.ctypes.data_as(C.c_void_p), C.c_uint32(2 * tw.size))
    if code != 0:
        raise M17HipError(f"m17hip_wide_spectrum_twiddles: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return tw


def wide_spectrum_carriers(power, rate_hz, width_hz=9000.0, margin_db=10.0):
    """The carriers of a spectrum plane (Context.wide_spectrum_fetch) of sources at `rate_hz` samples per second.  Per source: the BAND POWER of bin k is the
    circular sum of the 2 h + 1 bins around it, h = round(width_hz / 2 / (rate_hz / N)); the floor is the row's median times 2 h + 1; peaks of the band
    power are picked greedily, strongest first, while they stand more than `margin_db` dB over the floor, and each excludes the bins within width_hz of
    itself — a bin from which the band power still rises, half a band at a time, into what a taken peak excludes is that peak's shoulder and is passed
    over; a peak's offset is the centroid over its band of what the bins hold above the row's median.  Returns (source, offset in Hz from the source's
    centre, signed in [-rate_hz / 2, rate_hz / 2), dB of the band power over the floor), strongest first — wide_fcw takes the offset as it is.  A row whose
    median is 0 or not finite reports nothing.  Pure numpy."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim == 1:
        p = p[None, :]
    N = p.shape[1]
    df = float(rate_hz) / N
    h = min(int(round(float(width_hz) / 2.0 / df)), (N - 1) // 2)
    nb = 2 * h + 1
    excl = int(np.ceil(float(width_hz) / df))
    d = np.arange(-h, h + 1)
    out = []
    for s in range(p.shape[0]):
        med = float(np.median(p[s]))
        if not np.isfinite(med) or med <= 0.0:
            continue
        with np.errstate(invalid="ignore"):
            cs = np.concatenate([[0.0], np.cumsum(np.concatenate([p[s, N - h:], p[s], p[s, :h]]))])
            band = cs[nb:] - cs[:-nb]   # band[k]: bins k - h .. k + h, circular
        floor = med * nb
        free = np.isfinite(band)
        need = floor * 10.0 ** (float(margin_db) / 10.0)
        while free.any():
            k = int(np.argmax(np.where(free, band, -np.inf)))
            if not band[k] > need:
                break
            j = k   # (uphill within half a band at a time: a shoulder of a peak already taken ends inside what that peak excludes, and is no peak)
            while True:
                near = (j + d) % N
                m = int(near[np.argmax(band[near])])
                if not band[m] > band[j]:
                    break
                j = m
            if j != k:
                free[k] = False
                continue
            w = np.maximum(p[s, (k + d) % N] - med, 0.0)
            c = (k if k < N // 2 else k - N) + (float((d * w).sum() / w.sum()) if w.sum() > 0.0 else 0.0)
            hz = (c * df + float(rate_hz) / 2.0) % float(rate_hz) - float(rate_hz) / 2.0
            out.append((s, hz, 10.0 * float(np.log10(band[k] / floor))))
            free[(k + np.arange(-excl, excl + 1)) % N] = False
    out.sort(key=lambda e: -e[2])
    return out


def synth_wide_k(hz_per_unit=0.0, p=1):
    """The deviation word of Context.synth_wide_config for a deviation of hz_per_unit Hz per int16 unit of the baseband at 48000 * p / q samples per
    second: 2^63 hz_per_unit / (48000 p^2) rounded half up; 0 selects M17's 2400 / (3 * 7168) — m17hip_synth_wide_k (no context, no GPU)."""
    k = C.c_uint64(0)
    code = load_library().m17hip_synth_wide_k(C.c_double(hz_per_unit), C.c_uint32(p), C.byref(k))
    if code != 0:
        raise M17HipError(f"m17hip_synth_wide_k: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return int(k.value)


def wide_meter_counts(first_output, outputs, window):
    """m_k, the outputs in every piece of a metered block (Context.wide_meter_fetch): the block of `outputs` outputs that begins at output `first_output`
    of the feed, cut where the feed's output index is a multiple of `window`.  int64 [K]; pure Python integers, any 64-bit first_output."""
    n0, t, w = int(first_output), int(outputs), int(window)
    if t < 1 or w < 1 or n0 < 0:
        raise ValueError("wide_meter_counts: outputs and window are at least 1, first_output at least 0")
    a0 = n0 % w
    k = (a0 + t - 1) // w + 1
    return np.array([min((j + 1) * w - a0, t) - max(j * w - a0, 0) for j in range(k)], dtype=np.int64)


def wide_meter_report(planes, counts, gain):
    """What the sums of a metered block mean, in float64: planes [3][C][K] (Context.wide_meter_fetch), counts [K] (wide_meter_counts) and the `gain` of the
    upload call give a dict of three [C][K] arrays —
        level_db      10 log10(sum p / m): the power of the channel's z, dB over an amplitude of 1 in the units of the source's samples
        offset_hz     (sum y / m) * 48000 / (2 pi gain): the carrier's offset from the channel's frequency word
        deviation_hz  sqrt(max(sum e / m - (sum y / m)^2, 0)) * 48000 / (2 pi gain): the spread of the discriminator's output, as a frequency
    A piece of a window gives that piece's figures; add the planes and the counts of a window's two pieces before the call for the window's."""
    pl = np.asarray(planes, dtype=np.float64)
    m = np.asarray(counts, dtype=np.float64).reshape(1, -1)
    if pl.ndim != 3 or pl.shape[0] != 3 or pl.shape[2] != m.shape[1]:
        raise ValueError("wide_meter_report: planes is [3][C][K] and counts [K]")
    hz = 48000.0 / (2.0 * np.pi * float(gain))
    mean_y = pl[1] / m
    with np.errstate(divide="ignore", invalid="ignore"):
        level = 10.0 * np.log10(pl[0] / m)
    return {"level_db": level, "offset_hz": mean_y * hz, "deviation_hz": np.sqrt(np.maximum(pl[2] / m - mean_y * mean_y, 0.0)) * hz}


def wide_squelch_half_bins(width_hz, rate_hz, points):
    """half_bins of Context.wide_squelch for a band of width_hz around a channel's word in a spectrum of `points` bins of sources at rate_hz samples per
    second: round(width_hz / 2 / (rate_hz / points)) — the h of wide_spectrum_carriers —, at most (points - 1) // 2 and at most 64, the limit of
    m17hip_wide_squelch: at fine bins (9 kHz at 4096 points and 240 kSPS would be 77) the band is then narrower than asked for; take fewer points."""
    n = int(points)
    return min(int(round(float(width_hz) / 2.0 / (float(rate_hz) / n))), (n - 1) // 2, 64)


def wide_squelch_levels(power, frames, half_bins, open_db, close_db):
    """(open_level, close_level) float32 [sources] of Context.wide_squelch from a fetched spectrum plane (Context.wide_spectrum_fetch: power [sources][points]
    of `frames` frames): per source the floor of a band of 2 half_bins + 1 bins PER FRAME — the row's median times 2 half_bins + 1, divided by frames —
    times 10^(open_db / 10) and 10^(close_db / 10).  The median is the floor while fewer than half the bins hold a carrier.  Computed in float64 and rounded
    to float32 once.  Pure numpy."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim == 1:
        p = p[None, :]
    if int(frames) < 1:
        raise ValueError("wide_squelch_levels: a plane of at least one frame")
    floor = np.median(p, axis=1) * (2 * int(half_bins) + 1) / float(int(frames))
    return ((floor * 10.0 ** (float(open_db) / 10.0)).astype(np.float32), (floor * 10.0 ** (float(close_db) / 10.0)).astype(np.float32))


def wide_squelch_ratio(db):
    """A ratio of Context.wide_squelch_floor from a margin over the floor in dB: np.float32(10 ** (db / 10))."""
    return np.float32(10.0 ** (float(db) / 10.0))


SCAN_SLOT, SCAN_ASSIGNED, SCAN_HELD = 1, 2, 4   # the flags of Context.wide_scan_fetch


def wide_scan_guard_bins(width_hz, rate_hz, points):
    """The guard of Context.wide_scan for carriers `width_hz` wide on sources of `rate_hz` samples per second and a spectrum of `points` bins:
    ceil(width_hz / (rate_hz / points)), at least 3 and at most points / 4 (what m17hip_wide_scan takes)."""
    x = int(np.ceil(float(width_hz) / (float(rate_hz) / int(points))))
    return max(3, min(x, int(points) // 4))


def wide_scan_hz(fcw, rate_hz):
    """The offsets in Hz (float64) of frequency words (Context.wide_scan_fetch) on sources of `rate_hz` samples per second: fcw * rate_hz / 2^32."""
    return np.asarray(fcw, dtype=np.int64).astype(np.int32).astype(np.float64) * (float(rate_hz) / 4294967296.0)


def wide_fcw(offset_hz, decim):
    """The signed 32-bit frequency word of an offset in Hz at 48000 * decim samples per second, rounded to the nearest word (wide_channels).  `decim` need
    not be an integer: under wide_resample it is decim1 * down / up."""
    w = int(round(float(offset_hz) / (48000.0 * decim) * 4294967296.0))
    return (w + (1 << 31)) % (1 << 32) - (1 << 31)


def _wide_array(a):
    """(format, contiguous [S][W]... array) of a numpy wideband block: complex64 [S][W], int16 or uint8 [S][W][2]; a single source may leave [S] out."""
    if a.dtype == np.complex64 and a.ndim in (1, 2):
        return IQ_F32, np.ascontiguousarray(a if a.ndim == 2 else a[None, :])
    if a.dtype in (np.int16, np.uint8) and a.ndim in (2, 3) and a.shape[-1] == 2:
        return (IQ_I16 if a.dtype == np.int16 else IQ_U8), np.ascontiguousarray(a if a.ndim == 3 else a[None, :, :])
    raise TypeError("a wideband block is complex64 [S][W], or int16 / uint8 [S][W][2]")


def comm_get_id():
    """128-byte RCCL id (rank 0 calls this and hands the bytes to the other ranks)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    code = load_library().m17hip_comm_get_id(buf)
    if code != 0:
        raise M17HipError(f"m17hip_comm_get_id: {load_library().m17hip_strerror(C.c_int(code)).decode()}")
    return buf.raw


class Comm:
    """RCCL communicator of one rank (one context = one GPU = one rank); creation is collective."""

    def __init__(self, ctx, comm_id, rank, nranks):
        self.lib, self.ctx, self.rank, self.nranks = ctx.lib, ctx, int(rank), int(nranks)
        self.h = C.c_void_p()
        ctx._chk(self.lib.m17hip_comm_create(ctx.h, C.c_char_p(bytes(comm_id)), C.c_int(rank), C.c_int(nranks), C.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.m17hip_comm_destroy(self.h)
            self.h = C.c_void_p()


class Context:
    """One demodulation context = `channels` independent 48 kSPS channels on one GPU (include/m17hip.h)."""

    _warned = False

    def __init__(self, max_channels, max_samples, device=0, stream=None):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.max_channels, self.max_samples = int(max_channels), int(max_samples)
        self._chk(self.lib.m17hip_ctx_create(C.c_int(device), C.c_uint32(max_channels), C.c_uint32(max_samples), C.byref(self.h)))
        if stream is not None:
            self.set_stream(stream)
        if not Context._warned and self.lib.m17hip_advice(self.h) & 3:
            Context._warned = True
            import warnings
            warnings.warn("m17hip: fewer than 16 hardware queues were asked for (GPU_MAX_HW_QUEUES) — with several contexts the streams will share "
                          "hardware queues and serialise; export GPU_MAX_HW_QUEUES=16 before the process touches the GPU (include/m17hip.h)")

    def _chk(self, code):
        if code != 0:
            hip = self.lib.m17hip_last_hip_error(self.h) if self.h else 0
            raise M17HipError(f"m17hip error {code}: {self.lib.m17hip_strerror(C.c_int(code)).decode()} (hip error {hip})")

    def close(self):
        if self.h:
            self.lib.m17hip_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        self._chk(self.lib.m17hip_set_stream(self.h, C.c_void_p(int(stream_handle))))

    @property
    def stream(self):
        """The context's main stream (a hipStream_t as an int): the library's own unless set_stream named another (m17hip_get_stream)."""
        h = C.c_void_p()
        self._chk(self.lib.m17hip_get_stream(self.h, C.byref(h)))
        return h.value or 0

    def torch_stream(self):
        """The main stream as a torch.cuda.ExternalStream: `with torch.cuda.stream(ctx.torch_stream()): ...` puts the host's tensor work in order
        with the context's."""
        import torch
        return torch.cuda.ExternalStream(self.stream)

    # ---- input -------------------------------------------------------------------------------------------------
    def upload(self, samples):
        """The input of the next run.  A float32 array is a float stream's input — samples in the reference's units, taken as they are
        (m17hip_upload_f32); anything else is int16 input, as ever."""
        if getattr(samples, "dtype", None) == np.float32:
            s = np.ascontiguousarray(samples)
            fn = self.lib.m17hip_upload_f32
        else:
            s = np.ascontiguousarray(samples, dtype=np.int16)
            fn = self.lib.m17hip_upload_i16
        if s.ndim == 1:
            s = s[None, :]
        self.C, self.T = s.shape
        self._chk(fn(self.h, _ptr(s), C.c_uint32(self.C), C.c_uint32(self.T), C.c_size_t(self.T)))

    def _by_dtype(self, stem, dtype):
        """The entry point `m17hip_upload_<i16|f32><stem>` for samples of `dtype` (int16, the default, or float32)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.int16), np.dtype(np.float32)):
            raise TypeError(f"input samples are int16 or float32, not {dt}")
        return getattr(self.lib, f"m17hip_upload_{'f32' if dt == np.float32 else 'i16'}{stem}")

    def upload_async(self, host_ptr, channels, samples, pitch=None, dtype=np.int16):
        """Stage the input of the NEXT run (pinned host memory at `host_ptr`, kept alive by the caller) while the current run computes."""
        self.C, self.T = int(channels), int(samples)
        self._chk(self._by_dtype("_async", dtype)(self.h, C.c_void_p(int(host_ptr)), C.c_uint32(self.C), C.c_uint32(self.T),
                                                  C.c_size_t(self.T if pitch is None else pitch)))

    def upload_device_async(self, dev_ptr, channels, samples, pitch=None, dtype=np.int16):
        """Stage the input of the NEXT run from device memory at `dev_ptr` (kept alive and unmodified by the caller until upload_wait)."""
        self.C, self.T = int(channels), int(samples)
        self._chk(self._by_dtype("_device_async", dtype)(self.h, C.c_void_p(int(dev_ptr)), C.c_uint32(self.C), C.c_uint32(self.T),
                                                         C.c_size_t(self.T if pitch is None else pitch)))

    # ---- complex IQ input: the FM discriminator on the device (m17hip_upload_iq*) ---------------------------------
    def upload_iq(self, samples, gain=1.0):
        """The input of the next run as complex IQ, one narrowband 48 kSPS stream per channel: gain * arg(x[n] conj(x[n-1])) goes into the float
        input slab (a float stream from there on; download_f32 returns it).  `samples`: numpy complex64 [C][T], numpy int16 [C][T][2] (I, Q), or a
        torch tensor of either ON THE DEVICE, which is read where it lies (m17hip_upload_iq_device).  The context's streams are non-blocking and do
        not wait for the stream that produced the tensor: it must be COMPLETE when this is called (torch.cuda.synchronize(), or the producer's
        stream synchronised).  IQ blocks continue one another per channel in call order; reset() / reset_channels() start a feed over."""
        if hasattr(samples, "data_ptr"):   # a torch tensor
            t = samples
            if not t.is_cuda:
                return self.upload_iq(t.numpy(), gain)
            if t.is_complex():
                if str(t.dtype) != "torch.complex64":
                    raise TypeError(f"IQ samples are complex64 or int16 pairs, not {t.dtype}")
                if t.dim() == 1:
                    t = t[None, :]
                fmt = IQ_F32
            else:
                if str(t.dtype) != "torch.int16" or t.shape[-1] != 2:
                    raise TypeError("IQ samples are complex64 [C][T] or int16 [C][T][2]")
                if t.dim() == 2:
                    t = t[None, :, :]
                fmt = IQ_I16
            t = t.contiguous()   # (the call below has read it when it returns)
            return self.upload_iq_device(t.data_ptr(), int(t.shape[0]), int(t.shape[1]), iq_format=fmt, gain=gain)
        a = np.asarray(samples)
        if a.dtype == np.complex64:
            a = np.ascontiguousarray(a)
            if a.ndim == 1:
                a = a[None, :]
            fmt = IQ_F32
        elif a.dtype == np.int16 and a.ndim >= 2 and a.shape[-1] == 2:
            a = np.ascontiguousarray(a)
            if a.ndim == 2:
                a = a[None, :, :]
            fmt = IQ_I16
        else:
            raise TypeError("IQ samples are complex64 [C][T] or int16 [C][T][2]")
        self.C, self.T = int(a.shape[0]), int(a.shape[1])
        self._chk(self.lib.m17hip_upload_iq(self.h, _ptr(a), C.c_int(fmt), C.c_float(gain), C.c_uint32(self.C), C.c_uint32(self.T), C.c_size_t(self.T)))

    def _upload_iq_raw(self, name, ptr, channels, samples, pitch, iq_format, gain):
        self.C, self.T = int(channels), int(samples)
        self._chk(getattr(self.lib, name)(self.h, C.c_void_p(int(ptr)), C.c_int(iq_format), C.c_float(gain), C.c_uint32(self.C), C.c_uint32(self.T),
                                          C.c_size_t(self.T if pitch is None else pitch)))

    def upload_iq_async(self, host_ptr, channels, samples, pitch=None, iq_format=IQ_F32, gain=1.0):
        """Stage the NEXT run's input from IQ in pinned host memory (pitch in complex samples; kept alive and unmodified until upload_wait)."""
        self._upload_iq_raw("m17hip_upload_iq_async", host_ptr, channels, samples, pitch, iq_format, gain)

    def upload_iq_device(self, dev_ptr, channels, samples, pitch=None, iq_format=IQ_F32, gain=1.0):
        """IQ in device memory, complete when the call is made; the discriminator has read it when this returns."""
        self._upload_iq_raw("m17hip_upload_iq_device", dev_ptr, channels, samples, pitch, iq_format, gain)

    def upload_iq_device_async(self, dev_ptr, channels, samples, pitch=None, iq_format=IQ_F32, gain=1.0):
        """Stage the NEXT run's input from IQ in device memory (complete when the call is made; kept alive and unmodified until upload_wait)."""
        self._upload_iq_raw("m17hip_upload_iq_device_async", dev_ptr, channels, samples, pitch, iq_format, gain)

    # ---- wideband IQ input: the tuner on the device (m17hip_wide_*, m17hip_upload_wide*) ------------------------
    def wide_config(self, sources, decim, fmt=None, taps=None):
        """`sources` wide IQ streams at 48000 * decim samples per second in format `fmt` (IQ_I16 — the default —, IQ_F32, IQ_U8), low-passed with
        `taps` (None: wide_default_taps(decim)).  Starts every source's feed over; may be called again — m17hip_wide_config."""
        t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self._chk(self.lib.m17hip_wide_config(self.h, C.c_uint32(sources), C.c_uint32(decim), C.c_int(IQ_I16 if fmt is None else fmt), _ptr(t),
                                              C.c_uint32(0 if t is None else t.size)))
        self._wide = (int(sources), int(decim), IQ_I16 if fmt is None else int(fmt))
        self._wide_up = 1

    def wide_config2(self, sources, decim1, decim2, fmt=None, taps1=None, taps2=None):
        """`sources` wide IQ streams at 48000 * decim1 * decim2 samples per second (each 1..16) in format `fmt`, decimated in two stages: low-passed with
        `taps1` and every decim1-th sample kept, then with `taps2` and every decim2-th (None: that stage of wide_default_taps2(decim1, decim2)).  Replaces
        wide_config and is replaced by it; the frequency words are wide_fcw(offset_hz, decim1 * decim2) — m17hip_wide_config2."""
        t1 = None if taps1 is None else np.ascontiguousarray(taps1, dtype=np.float32).reshape(-1)
        t2 = None if taps2 is None else np.ascontiguousarray(taps2, dtype=np.float32).reshape(-1)
        self._chk(self.lib.m17hip_wide_config2(self.h, C.c_uint32(sources), C.c_uint32(decim1), _ptr(t1), C.c_uint32(0 if t1 is None else t1.size),
                                               C.c_uint32(decim2), _ptr(t2), C.c_uint32(0 if t2 is None else t2.size), C.c_int(IQ_I16 if fmt is None else fmt)))
        self._wide = (int(sources), int(decim1) * int(decim2), IQ_I16 if fmt is None else int(fmt))
        self._wide_up = 1

    def wide_resample(self, sources, decim1, up, down, fmt=None, taps1=None, taps2=None):
        """`sources` wide IQ streams at 48000 * decim1 * down / up samples per second (decim1 1..16, up 1..32, down 1..125, up <= down and coprime:
        wide_resample_ratio finds them for a rate) in format `fmt`: low-passed with `taps1` and every decim1-th sample kept, then resampled by up / down
        through `taps2` (None: that stage of wide_resample_default_taps(decim1, up, down)).  Replaces the other three configurations and is replaced by
        them; the frequency words are wide_fcw(offset_hz, decim1 * down / up); a block holds a multiple of `up` outputs — m17hip_wide_resample."""
        t1 = None if taps1 is None else np.ascontiguousarray(taps1, dtype=np.float32).reshape(-1)
        t2 = None if taps2 is None else np.ascontiguousarray(taps2, dtype=np.float32).reshape(-1)
        self._chk(self.lib.m17hip_wide_resample(self.h, C.c_uint32(sources), C.c_uint32(decim1), _ptr(t1), C.c_uint32(0 if t1 is None else t1.size),
                                                C.c_uint32(up), C.c_uint32(down), _ptr(t2), C.c_uint32(0 if t2 is None else t2.size),
                                                C.c_int(IQ_I16 if fmt is None else fmt)))
        self._wide = (int(sources), int(decim1) * int(down), IQ_I16 if fmt is None else int(fmt))   # (samples per group of `up` outputs)
        self._wide_up = int(up)

    def wide_raster(self, sources, decim, bins, fmt=None, taps=None):
        """`sources` wide IQ streams at 48000 * decim samples per second (decim 1..64) in format `fmt`, every one split into `bins` channels spaced
        48000 * decim / bins Hz by the polyphase channeliser, low-passed with `taps` (None: wide_raster_default_taps(decim)).  Replaces wide_config and
        wide_config2 and is replaced by them; channels are named by wide_raster_channels — m17hip_wide_raster."""
        t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        self._chk(self.lib.m17hip_wide_raster(self.h, C.c_uint32(sources), C.c_uint32(decim), C.c_uint32(bins), C.c_int(IQ_I16 if fmt is None else fmt),
                                              _ptr(t), C.c_uint32(0 if t is None else t.size)))
        self._wide = (int(sources), int(decim), IQ_I16 if fmt is None else int(fmt))
        self._wide_up = 1
        self._wide_bins = int(bins)

    def wide_raster_channels(self, source, bin):
        """Local channel c listens to bin[c] (wide_bin; -bins / 2 <= bin < bins / 2) of source[c] from the blocks uploaded after this call; several
        channels may name the same one — m17hip_wide_raster_channels."""
        src = np.ascontiguousarray(np.asarray(source, dtype=np.uint32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(bin, dtype=np.int64).reshape(-1).astype(np.int32))
        if src.size != b.size:
            raise ValueError("one source and one bin per channel")
        self._chk(self.lib.m17hip_wide_raster_channels(self.h, _ptr(src) if src.size else None, b.ctypes.data_as(C.c_void_p) if b.size else None,
                                                       C.c_uint32(src.size)))

    def wide_survey(self, stride):
        """The raster survey: from the blocks uploaded after this call, every `stride`-th output of the feed (1..4096; 0: off, the default) adds the power
        of EVERY bin of every source to the block's plane, listened to or not — m17hip_wide_survey.  Any wide_config / wide_config2 / wide_raster call
        turns it off."""
        self._chk(self.lib.m17hip_wide_survey(self.h, C.c_uint32(stride)))

    def wide_survey_fetch(self, back=0):
        """(power float32 [sources][bins] indexed by bin mod bins, survey times in the block, the feed's output index at the block's start) of the latest
        block uploaded with the survey on (back = 0) or the one before it (back = 1); waits for that block's survey kernels only —
        m17hip_wide_survey_fetch.  wide_raster_occupied reads the plane."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_survey_fetch: back is 0 or 1")
        cap = 256 * 256
        buf = np.zeros(cap, dtype=np.float32)
        times, first = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.m17hip_wide_survey_fetch(self.h, C.c_uint32(back), _ptr(buf), C.c_uint64(cap), C.byref(times), C.byref(first)))
        S, M = self._wide[0], self._wide_bins   # (the call succeeded: wide_raster has set both)
        return buf[: S * M].reshape(S, M).copy(), int(times.value), int(first.value)

    def wide_spectrum(self, points, hop, window=None):
        """The source spectrum: from the blocks uploaded after this call, every source block's frames of `points` samples (a power of two in 64..4096; 0:
        off, the default) that begin where the feed's sample index is a multiple of `hop` (1..2^24) are windowed (float32 [points]; None: the default
        Blackman-Harris window), transformed, and their powers summed into the block's plane — m17hip_wide_spectrum.  Legal under every wideband
        configuration; any wide_config / wide_config2 / wide_raster / wide_resample call turns it off."""
        w = None if window is None else np.ascontiguousarray(np.asarray(window, dtype=np.float32).reshape(-1))
        self._chk(self.lib.m17hip_wide_spectrum(self.h, C.c_uint32(points), C.c_uint32(hop), _ptr(w), C.c_uint32(0 if w is None else w.size)))
        self._spectrum_points = int(points)

    def wide_spectrum_fetch(self, back=0):
        """(power float32 [sources][points] — bin k at k * rate / points below points / 2, (k - points) * rate / points from there on —, frames in the block,
        the feed's sample index at the block's first frame) of the latest block uploaded with the spectrum on (back = 0) or the one before it (back = 1);
        waits for that block's spectrum kernels only — m17hip_wide_spectrum_fetch.  wide_spectrum_carriers reads the plane."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_spectrum_fetch: back is 0 or 1")
        S, N = getattr(self, "_wide", (0,))[0], getattr(self, "_spectrum_points", 0)   # (0 where wide_spectrum was never called: the library then refuses)
        buf = np.zeros(max(S * N, 1), dtype=np.float32)
        frames, first = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.m17hip_wide_spectrum_fetch(self.h, C.c_uint32(back), _ptr(buf), C.c_uint64(S * N), C.byref(frames), C.byref(first)))
        return buf.reshape(S, N), int(frames.value), int(first.value)

    def wide_meter(self, window):
        """The channel meter: from the blocks uploaded after this call, the sums of chan_power(z), of the discriminator's y and of y * y per channel and per
        window of `window` outputs of the feed (16..65536; 0: off, the default) — m17hip_wide_meter.  Legal under every wideband configuration; any
        wide_config / wide_config2 / wide_raster / wide_resample call turns it off; reset() keeps it on and starts the windows over."""
        self._chk(self.lib.m17hip_wide_meter(self.h, C.c_uint32(window)))

    def wide_meter_fetch(self, back=0):
        """(planes float32 [3][C][K] — sum p, sum y, sum y * y of channel c over piece k —, first_window, first_output, outputs) of the latest block
        uploaded with the meter on (back = 0) or the one before it (back = 1): piece k belongs to window first_window + k of the feed, the block began at
        output first_output and holds `outputs` outputs per channel (wide_meter_counts gives the pieces' counts, wide_meter_report the meaning).  Waits
        for that block's meter kernel only — m17hip_wide_meter_shape, m17hip_wide_meter_fetch."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_meter_fetch: back is 0 or 1")
        ch, k, t = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        fw, fo = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.m17hip_wide_meter_shape(self.h, C.c_uint32(back), C.byref(ch), C.byref(k), C.byref(fw), C.byref(fo), C.byref(t)))
        n = 3 * ch.value * k.value
        buf = np.zeros(max(n, 1), dtype=np.float32)
        self._chk(self.lib.m17hip_wide_meter_fetch(self.h, C.c_uint32(back), _ptr(buf), C.c_uint64(n)))
        return buf[:n].reshape(3, ch.value, k.value), int(fw.value), int(fo.value), int(t.value)

    def wide_squelch(self, half_bins, open_level, close_level=None, hang=0):
        """The spectrum squelch of the three tuners (wide_config, wide_config2, wide_resample; the spectrum must be on): from the blocks uploaded after this
        call a channel whose band — the 2 half_bins + 1 bins of the block's spectrum around its frequency word — lies below open_level[source] x frames is
        not tuned: its floats are +0.  A channel that was open stays open while the band is at least close_level x frames (None: the open level) and for
        `hang` blocks after that.  Scalars broadcast to all sources; open_level None turns it off (the default) — m17hip_wide_squelch.  Every wide_spectrum
        call and every configuration call turns it off; reset() keeps it on and clears the hold counts."""
        if open_level is None:
            self._chk(self.lib.m17hip_wide_squelch(self.h, C.c_uint32(0), None, None, C.c_uint32(0), C.c_uint32(0)))
            return
        S = getattr(self, "_wide", (0,))[0]
        o = np.asarray(open_level, dtype=np.float32).reshape(-1)
        cl = o if close_level is None else np.asarray(close_level, dtype=np.float32).reshape(-1)
        o = np.ascontiguousarray(np.repeat(o, S) if o.size == 1 and S > 1 else o)
        cl = np.ascontiguousarray(np.repeat(cl, S) if cl.size == 1 and S > 1 else cl)
        if o.size != cl.size:
            raise ValueError("one open and one close level per source")
        self._chk(self.lib.m17hip_wide_squelch(self.h, C.c_uint32(half_bins), _ptr(o), _ptr(cl), C.c_uint32(o.size), C.c_uint32(hang)))

    def wide_squelch_fetch(self, back=0):
        """(open bool [C], hold uint32 [C], band float32 [C], frames) of the latest block uploaded with the squelch on (back = 0) or the one before it
        (back = 1): whether the block's channel was tuned, its hold count behind the block, the band power the decision was made from and the spectrum's
        frame count of the block.  Waits for that block's squelch kernel only — m17hip_wide_squelch_fetch."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_squelch_fetch: back is 0 or 1")
        cap = max(self.max_channels, 1)
        state, band = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.float32)
        n, frames = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.lib.m17hip_wide_squelch_fetch(self.h, C.c_uint32(back), _ptr(state), _ptr(band), C.c_uint64(cap), C.byref(n), C.byref(frames)))
        state, band = state[: n.value], band[: n.value].copy()
        return (state >> 31).astype(bool), state & np.uint32(0x7FFFFFFF), band, int(frames.value)

    def wide_squelch_slots(self, half_bins, open_level, close_level=None, hang=0, lead=0):
        """The time-resolved mode of the squelch, exclusive with wide_squelch's: the decision is taken per SLOT of a block — 16 frames of its spectrum — with
        `hang` counted in slots, and the tuners skip per TILE of outputs (255, or groups x up under wide_resample); `lead` (0..255) opens the tiles in front
        of an opening within the block.  Levels as wide_squelch's (wide_squelch_levels serves: they are per frame); open_level None turns the squelch off
        whichever mode was on — m17hip_wide_squelch_slots."""
        if open_level is None:
            self._chk(self.lib.m17hip_wide_squelch_slots(self.h, C.c_uint32(0), None, None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)))
            return
        S = getattr(self, "_wide", (0,))[0]
        o = np.asarray(open_level, dtype=np.float32).reshape(-1)
        cl = o if close_level is None else np.asarray(close_level, dtype=np.float32).reshape(-1)
        o = np.ascontiguousarray(np.repeat(o, S) if o.size == 1 and S > 1 else o)
        cl = np.ascontiguousarray(np.repeat(cl, S) if cl.size == 1 and S > 1 else cl)
        if o.size != cl.size:
            raise ValueError("one open and one close level per source")
        self._chk(self.lib.m17hip_wide_squelch_slots(self.h, C.c_uint32(half_bins), _ptr(o), _ptr(cl), C.c_uint32(o.size), C.c_uint32(hang), C.c_uint32(lead)))

    def wide_squelch_slots_fetch(self, back=0):
        """(state uint32 [C], bands float32 [C][G], mask uint32 [C][ceil(tiles / 32)], tiles, frames) of the latest block uploaded in slot mode (back = 0) or the
        one before it (back = 1): the channels' state words behind the block (hold | open << 31 of the last slot), the band power of every slot, the tile
        mask the tuner read (bit t & 31 of word t >> 5 set: tile t tuned) and the block's tile and frame counts.  Waits for that block's squelch kernels only —
        m17hip_wide_squelch_slots_fetch.  The plane sizes are the block's, so the call is repeated with larger buffers while the library refuses them."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_squelch_slots_fetch: back is 0 or 1")
        cap = max(self.max_channels, 1)
        per = 64
        while True:
            state, bands, mask = np.zeros(cap, dtype=np.uint32), np.zeros(cap * per, dtype=np.float32), np.zeros(cap * per, dtype=np.uint32)
            n, g, t, frames = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            rc = self.lib.m17hip_wide_squelch_slots_fetch(self.h, C.c_uint32(back), _ptr(state), _ptr(bands), _ptr(mask), C.c_uint64(cap), C.c_uint64(cap * per),
                                                          C.c_uint64(cap * per), C.byref(n), C.byref(g), C.byref(t), C.byref(frames))
            if rc == -1 and per < (1 << 22):   # (M17HIP_EINVAL: the only argument that can be wrong here is a capacity)
                per *= 8
                continue
            self._chk(rc)
            break
        c, mw = n.value, (t.value + 31) // 32
        return (state[:c].copy(), bands[: c * g.value].reshape(c, g.value).copy(), mask[: c * mw].reshape(c, mw).copy(), int(t.value), int(frames.value))

    def wide_squelch_floor(self, open_ratio, close_ratio, rise=1.0, fall=1.0, floor_min=0.0):
        """The sources' noise floor on the device, beside whichever squelch mode is on (wide_squelch or wide_squelch_slots first; its half_bins, hang and
        lead stay, its given levels are set aside): from the blocks uploaded after this call a kernel in front of the squelch takes each source's floor from
        the block's own plane — the row's upper median times 2 half_bins + 1 over the frames, at least floor_min —, tracks it from block to block (towards a
        higher floor by `rise`, towards a lower one by `fall`, both in (0, 1]; 1 follows at once) and the block's levels are the tracked floor times
        open_ratio and close_ratio (wide_squelch_ratio(dB)).  open_ratio == close_ratio == 0 turns it off: the given levels serve again.  Every
        wide_squelch and wide_squelch_slots call turns it off — m17hip_wide_squelch_floor."""
        self._chk(self.lib.m17hip_wide_squelch_floor(self.h, C.c_float(open_ratio), C.c_float(close_ratio), C.c_float(rise), C.c_float(fall), C.c_float(floor_min)))

    def wide_squelch_floor_fetch(self, back=0):
        """(plane float32 [4][S], frames) of the latest block uploaded with wide_squelch_floor on (back = 0) or the one before it (back = 1): per source the
        plane's median, the tracked floor behind the block, and the open and close levels the squelch read.  Waits for that block's floor and squelch
        kernels only — m17hip_wide_squelch_floor_fetch."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_squelch_floor_fetch: back is 0 or 1")
        buf = np.zeros(4 * 256, dtype=np.float32)
        n, frames = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.lib.m17hip_wide_squelch_floor_fetch(self.h, C.c_uint32(back), _ptr(buf), C.c_uint64(buf.size), C.byref(n), C.byref(frames)))
        return buf[: 4 * n.value].reshape(4, n.value).copy(), int(frames.value)

    def wide_scan(self, pool, guard_bins=None, rate_hz=None):
        """The carrier scan, beside wide_spectrum (at most 4096 points), wide_squelch and wide_squelch_floor: `pool` is an array-like of 0 / 1 for local
        channels 0 .. len - 1, a 1 makes the channel a SLOT of the source its wide_channels entry names.  From the blocks uploaded after this call a kernel
        in front of the squelch finds the carriers of each source's block and writes the frequency words of the source's slots that are not held by a
        carrier already: a transmission is tuned in the block in which it first appears.  guard_bins (3 .. points / 4) is the least distance of two
        carriers; None takes wide_scan_guard_bins(9000, rate_hz, points) — `rate_hz` the sources' sample rate, by default the configuration's 48000 x
        decimation.  pool None turns it off.  run() then resets the channels a block has just assigned before it queues the run — m17hip_wide_scan."""
        if pool is None:
            self._chk(self.lib.m17hip_wide_scan(self.h, None, C.c_uint32(0), C.c_uint32(0)))
            self._scan = False
            return
        a = np.ascontiguousarray((np.asarray(pool).reshape(-1) != 0).astype(np.uint8))
        if guard_bins is None:
            points, (_, R, _) = getattr(self, "_spectrum_points", 0), getattr(self, "_wide", (0, 0, 0))
            rate = rate_hz or 48000.0 * R / getattr(self, "_wide_up", 1)   # (the configuration's own rate)
            guard_bins = wide_scan_guard_bins(9000.0, rate, points) if rate and points else 3
        self._chk(self.lib.m17hip_wide_scan(self.h, _ptr(a) if a.size else None, C.c_uint32(a.size), C.c_uint32(guard_bins)))
        self._scan = True
        self._scan_pending = False

    def wide_scan_fetch(self, back=0):
        """(fcw int32 [C], flags uint32 [C], missed uint32 [S], assigned) of the latest block uploaded with wide_scan on (back = 0) or the one before it
        (back = 1): the frequency words the block was tuned with, per channel SCAN_SLOT | SCAN_ASSIGNED (in this block) | SCAN_HELD (a carrier it had
        holds it), per source the carriers that found no free slot, and the list of the channels assigned in this block.  Waits for that block's scan
        kernel only — m17hip_wide_scan_fetch."""
        if back not in (0, 1):
            raise M17HipError("m17hip_wide_scan_fetch: back is 0 or 1")
        cap = max(self.max_channels, 1)
        fcw, flags, missed = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
        n, srcs, frames = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._chk(self.lib.m17hip_wide_scan_fetch(self.h, C.c_uint32(back), fcw.ctypes.data_as(C.c_void_p), _ptr(flags), _ptr(missed), C.c_uint64(cap),
                                                  C.byref(n), C.byref(srcs), C.byref(frames)))
        fcw, flags = fcw[: n.value].copy(), flags[: n.value].copy()
        return fcw, flags, missed[: srcs.value].copy(), [int(c) for c in np.flatnonzero(flags & np.uint32(SCAN_ASSIGNED))]

    def wide_channels(self, source, fcw):
        """Local channel c listens to source[c] at the frequency word fcw[c] (wide_fcw) from the blocks uploaded after this call — m17hip_wide_channels."""
        src = np.ascontiguousarray(np.asarray(source, dtype=np.uint32).reshape(-1))
        w = np.ascontiguousarray(np.asarray(fcw, dtype=np.int64).reshape(-1).astype(np.int32))
        if src.size != w.size:
            raise ValueError("one source and one frequency word per channel")
        self._chk(self.lib.m17hip_wide_channels(self.h, _ptr(src) if src.size else None, w.ctypes.data_as(C.c_void_p) if w.size else None, C.c_uint32(src.size)))

    def upload_wide(self, x, gain=1.0, staged=False, channels=None):
        """The input of the next run from one block of every source: numpy complex64 [S][W], int16 or uint8 [S][W][2] (W = outputs * decim — under
        wide_resample outputs / up * down * decim1: a whole number of groups of down * decim1 samples, each `up` outputs —; the dtype must
        be the configured format), or a torch tensor of those ON THE DEVICE, COMPLETE when this is called (see upload_iq).  `channels` (default: the
        context's) are tuned, filtered, decimated and discriminated into the float input slab.  staged: for the NEXT run, on the copy stream (host memory
        then has to be pinned and kept unmodified until upload_wait; so has a device tensor)."""
        dev = hasattr(x, "data_ptr") and x.is_cuda
        if hasattr(x, "data_ptr"):
            kinds = {"torch.complex64": IQ_F32, "torch.int16": IQ_I16, "torch.uint8": IQ_U8}
            f = kinds.get(str(x.dtype))
            if f is None or (f != IQ_F32 and (x.dim() < 2 or x.shape[-1] != 2)) or (f == IQ_F32 and x.dim() not in (1, 2)):
                raise TypeError("a wideband block is complex64 [S][W], or int16 / uint8 [S][W][2]")
            if not dev:
                return self.upload_wide(x.numpy(), gain, staged, channels)
            a = x.contiguous()
            if (f == IQ_F32 and a.dim() == 1) or (f != IQ_F32 and a.dim() == 2):
                a = a[None]
            ptr = a.data_ptr()
        else:
            f, a = _wide_array(np.asarray(x))
            ptr = a.ctypes.data
        S, R, fmt = getattr(self, "_wide", (0, 0, 0))
        if not S:
            raise M17HipError("m17hip error -4: wide_config has not been called")
        if f != fmt or a.shape[0] != S or a.shape[1] == 0 or a.shape[1] % R:
            raise TypeError(f"a block of the configured format {fmt} with {S} sources and a multiple of {R} samples per source")
        self._keep = a   # (a staged block is read until upload_wait)
        name = "m17hip_upload_wide" + ("_device" if dev else "") + ("_async" if staged else "")
        self._upload_wide_raw(name, ptr, self.max_channels if channels is None else channels, a.shape[1] // R * getattr(self, "_wide_up", 1), a.shape[1], gain)

    def _upload_wide_raw(self, name, ptr, channels, samples, pitch, gain):
        self.C, self.T = int(channels), int(samples)
        self._chk(getattr(self.lib, name)(self.h, C.c_void_p(int(ptr)), C.c_float(gain), C.c_uint32(self.C), C.c_uint32(self.T), C.c_size_t(pitch)))
        self._scan_pending = getattr(self, "_scan", False)   # (wide_scan: run() resets what this block assigns)

    def upload_wide_async(self, host_ptr, channels, samples, pitch, gain=1.0):
        """Stage the NEXT run's input from a wideband block in pinned host memory (pitch in complex samples; kept unmodified until upload_wait)."""
        self._upload_wide_raw("m17hip_upload_wide_async", host_ptr, channels, samples, pitch, gain)

    def upload_wide_device(self, dev_ptr, channels, samples, pitch, gain=1.0):
        """A wideband block in device memory, complete when the call is made; the tuner has read it when this returns."""
        self._upload_wide_raw("m17hip_upload_wide_device", dev_ptr, channels, samples, pitch, gain)

    def upload_wide_device_async(self, dev_ptr, channels, samples, pitch, gain=1.0):
        """Stage the NEXT run's input from a wideband block in device memory (complete when the call is made; kept unmodified until upload_wait)."""
        self._upload_wide_raw("m17hip_upload_wide_device_async", dev_ptr, channels, samples, pitch, gain)

    def iq_bytes(self):
        """Device bytes the context holds for IQ input (the carry and the host forms' raw buffer); 0 if it has never seen IQ — m17hip_iq_bytes."""
        n = C.c_uint64(0)
        self._chk(self.lib.m17hip_iq_bytes(self.h, C.byref(n)))
        return n.value

    def input_alternate(self, channels=None, samples=None):
        """Stage, without a copy, the input the context's second slab still holds (two resident slabs that alternate)."""
        self._chk(self.lib.m17hip_input_alternate(self.h, C.c_uint32(channels or self.C), C.c_uint32(samples or self.T)))

    def front(self, flags=0, channels=None, samples=None):
        """Queue the front end (matched filter, carrier-detect sums) of the STAGED run now, beside the latest run's state-machine half;
        the run() that follows (same arguments) queues the rest."""
        self._chk(self.lib.m17hip_demod_front(self.h, C.c_uint32(channels or self.C), C.c_uint32(samples or self.T), C.c_uint32(flags)))

    def upload_wait(self):
        """Block until the copy queued by upload_async has left the host buffer."""
        self._chk(self.lib.m17hip_upload_wait(self.h))

    def synth(self, params, channels, samples, chan0=0):
        """Generate the input slab on the device (m17-mod framing + impairments); `params` = a ctypes block laid out as m17_synth_params."""
        self.C, self.T = int(channels), int(samples)
        self._chk(self.lib.m17hip_synth_i16(self.h, C.byref(params), C.c_uint32(self.C), C.c_uint32(self.T), C.c_uint32(chan0)))

    def synth_sweep(self, base, points, channels, samples, chan0=0):
        """An impairment sweep in one synthesis (m17hip_synth_sweep_i16): channel c under points[(chan0 + c) % len(points)], everything else
        from `base` (an m17_synth_params block).  `points`: an IMPAIRMENT_DTYPE array or a sequence of (noise_sigma, tail_sigma, dc_offset, gain)."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=IMPAIRMENT_DTYPE).reshape(-1))
        self.C, self.T = int(channels), int(samples)
        self._chk(self.lib.m17hip_synth_sweep_i16(self.h, C.byref(base), _ptr(pts), C.c_uint32(pts.size), C.c_uint32(self.C), C.c_uint32(self.T),
                                                  C.c_uint32(chan0)))

    def synth_tx(self, base, transmissions, samples, chan0=0):
        """Generate the input slab on the device from the caller's own transmissions, one per channel (m17hip_synth_tx_i16: the framing of
        apps/m17-mod.cpp:264-504, 509-564 with the content supplied).  A transmission is (kind, lsf_bytes_or_None, [row_bytes, ...]): kind
        TX_BERT / TX_STREAM / TX_PACKET, the 30-byte LSF sent as given (make_lsf; None for BERT), and one row of up to 32 bytes per payload
        frame (stream_row; 26 bytes of a packet frame; 25 of a BERT frame).  `base` = an m17_synth_params block: seed, lead_in, phase, invert,
        n_preamble and the impairments; its kind and n_frames are ignored."""
        tx = np.zeros(len(transmissions), dtype=TX_DTYPE)
        lsf = np.zeros((len(transmissions), 30), dtype=np.uint8)
        rows = []
        for i, (kind, lsf_bytes, frames) in enumerate(transmissions):
            tx[i] = (kind, len(frames), len(rows), 0)
            if lsf_bytes is not None:
                lsf[i] = np.frombuffer(bytes(lsf_bytes), dtype=np.uint8)   # (exactly 30 bytes)
            elif kind != TX_BERT:
                raise ValueError("a stream or packet transmission needs its LSF")
            for row in frames:
                row = bytes(row)
                if len(row) > 32:
                    raise ValueError("a row is 32 bytes at the most")
                rows.append(row.ljust(32, b"\0"))
        rows_arr = np.frombuffer(b"".join(rows), dtype=np.uint8) if rows else np.zeros(32, dtype=np.uint8)
        self._chk(self.lib.m17hip_synth_tx_i16(self.h, C.byref(base), _ptr(tx), _ptr(lsf), _ptr(rows_arr), C.c_uint32(len(rows)),
                                               C.c_uint32(len(transmissions)), C.c_uint32(int(samples)), C.c_uint32(chan0)))
        self.C, self.T = len(transmissions), int(samples)

    def synth_wide_config(self, sources, p, q=1, fmt=IQ_I16, k=None, noise_sigma=0.0, seed=0, first_sample=0):
        """Configure the wideband signal generator: `sources` streams at 48000 * p / q samples per second in the format `fmt`, the deviation word k (None:
        synth_wide_k(0, p), M17's deviation), noise of noise_sigma from `seed`, the feed's sample count beginning at first_sample (a multiple of p) —
        m17hip_synth_wide_config.  The table is fresh afterwards: nobody transmits."""
        k = synth_wide_k(0.0, p) if k is None else int(k)
        self._chk(self.lib.m17hip_synth_wide_config(self.h, C.c_uint32(sources), C.c_uint32(p), C.c_uint32(q), C.c_int(fmt), C.c_uint64(k),
                                                    C.c_float(noise_sigma), C.c_uint64(seed), C.c_uint64(first_sample)))
        self._wide_tx = (int(sources), int(p), int(q), int(fmt))

    def synth_wide_channels(self, source, fcw, phase0=0, amplitude=0.0):
        """Channel c transmits on source[c] at the frequency word fcw[c] (wide_fcw at the generator's rate, p / q) with the start phase phase0[c] and the
        amplitude amplitude[c] (scalars hold for every channel) from the next synth_wide call; channels past the sequences keep theirs —
        m17hip_synth_wide_channels.  A WIDE_TX_DTYPE array as `source` is taken as the table itself."""
        if isinstance(source, np.ndarray) and source.dtype == WIDE_TX_DTYPE:
            tx = np.ascontiguousarray(source.reshape(-1))
        else:
            src = np.asarray(source, dtype=np.uint32).reshape(-1)
            tx = np.zeros(src.size, dtype=WIDE_TX_DTYPE)
            tx["source"] = src
            tx["fcw"] = np.broadcast_to(np.asarray(fcw, dtype=np.int64), src.shape).astype(np.int32)
            tx["phase0"] = np.broadcast_to(np.asarray(phase0, dtype=np.int64) & 0xFFFFFFFF, src.shape).astype(np.uint32)
            tx["amplitude"] = np.broadcast_to(np.asarray(amplitude, dtype=np.float32), src.shape)
        self._chk(self.lib.m17hip_synth_wide_channels(self.h, tx.ctypes.data_as(C.c_void_p), C.c_uint32(tx.size)))

    def synth_wide(self, samples=None, out=None, channels=None):
        """One block of the generator from the int16 input the slab holds (`channels` x `samples`, default: the last input's; samples a multiple of q):
        W = samples / q * p complex samples per source.  out = None: a numpy array complex64 [S][W], or int16 / uint8 [S][W][2] — m17hip_synth_wide.
        out = a torch tensor ON THE DEVICE of that dtype and at least that shape ([S][pitch] complex64 or [S][pitch][2]), contiguous: filled in place,
        complete when this returns (what upload_wide / upload_wide_device ask of their producer) — m17hip_synth_wide_device."""
        S, P, Q, fmt = getattr(self, "_wide_tx", (0, 1, 1, IQ_I16))
        n = int(self.T if samples is None else samples)
        ch = int(self.C if channels is None else channels)
        W = n // Q * P
        if out is None:
            shape = (max(S, 1), max(W, 1))
            a = np.zeros(shape, dtype=np.complex64) if fmt == IQ_F32 else np.zeros(shape + (2,), dtype=np.int16 if fmt == IQ_I16 else np.uint8)
            self._chk(self.lib.m17hip_synth_wide(self.h, a.ctypes.data_as(C.c_void_p), C.c_uint32(ch), C.c_uint32(n), C.c_size_t(a.shape[1])))
            return a[:S, :W]
        kinds = {"torch.complex64": IQ_F32, "torch.int16": IQ_I16, "torch.uint8": IQ_U8}
        if not (hasattr(out, "data_ptr") and out.is_cuda and out.is_contiguous()) or kinds.get(str(out.dtype)) != fmt:
            raise TypeError("out is a contiguous device tensor of the configured format")
        if out.dim() != (2 if fmt == IQ_F32 else 3) or out.shape[0] < S or (fmt != IQ_F32 and out.shape[2] != 2):
            raise TypeError("out is complex64 [S][pitch], or int16 / uint8 [S][pitch][2]")
        self._chk(self.lib.m17hip_synth_wide_device(self.h, C.c_void_p(out.data_ptr()), C.c_uint32(ch), C.c_uint32(n), C.c_size_t(out.shape[1])))
        return out

    def download(self, channels=None):
        """The input slab's first `channels` rows (default: all of the last input)."""
        n = channels or self.C
        out = np.empty((n, self.T), dtype=np.int16)
        self._chk(self.lib.m17hip_download_i16(self.h, _ptr(out), C.c_uint32(n), C.c_uint32(self.T), C.c_size_t(self.T)))
        return out

    def download_f32(self, channels=None):
        """The float input slab's first `channels` rows (a float stream), byte for byte what was uploaded."""
        n = channels or self.C
        out = np.empty((n, self.T), dtype=np.float32)
        self._chk(self.lib.m17hip_download_f32(self.h, _ptr(out), C.c_uint32(n), C.c_uint32(self.T), C.c_size_t(self.T)))
        return out

    def input_format(self):
        """(the stream's sample format: 0 free / FORMAT_I16 / FORMAT_F32, device bytes held for float input) — m17hip_input_format."""
        fmt, nbytes = C.c_int(0), C.c_uint64(0)
        self._chk(self.lib.m17hip_input_format(self.h, C.byref(fmt), C.byref(nbytes)))
        return fmt.value, nbytes.value

    def upload_device(self, dev_ptr, channels, samples, pitch=None, dtype=np.int16):
        self.C, self.T = int(channels), int(samples)
        self._chk(self._by_dtype("_device", dtype)(self.h, C.c_void_p(int(dev_ptr)), C.c_uint32(self.C), C.c_uint32(self.T),
                                                  C.c_size_t(self.T if pitch is None else pitch)))

    # ---- per-operator entry points --------------------------------------------------------------------------------
    def fir(self, flags=0, fetch=True):
        out = np.empty((self.C, self.T), dtype=np.float32) if fetch else None
        self._chk(self.lib.m17hip_fir_rrc150(self.h, C.c_uint32(self.C), C.c_uint32(self.T), C.c_uint32(flags), _ptr(out)))
        return out

    def correlator(self):
        limit = np.empty((self.C, self.T), dtype=np.float32)
        corr = np.empty((4, self.C, self.T), dtype=np.float32)
        self._chk(self.lib.m17hip_correlator(self.h, C.c_uint32(self.C), C.c_uint32(self.T), _ptr(limit), _ptr(corr)))
        return limit, corr

    def fir_correlator(self, flags=0, fetch=True):
        """configs[1] as one call: matched filter + limit filter + the four correlations, pipelined in time (m17hip_fir_correlator)."""
        if not fetch:
            self._chk(self.lib.m17hip_fir_correlator(self.h, C.c_uint32(self.C), C.c_uint32(self.T), C.c_uint32(flags), None, None, None))
            return None
        y = np.empty((self.C, self.T), dtype=np.float32)
        limit = np.empty((self.C, self.T), dtype=np.float32)
        corr = np.empty((4, self.C, self.T), dtype=np.float32)
        self._chk(self.lib.m17hip_fir_correlator(self.h, C.c_uint32(self.C), C.c_uint32(self.T), C.c_uint32(flags), _ptr(y), _ptr(limit), _ptr(corr)))
        return y, limit, corr

    def correlator_device(self):
        """Same computation, results left in device memory (benchmarks)."""
        self._chk(self.lib.m17hip_correlator(self.h, C.c_uint32(self.C), C.c_uint32(self.T), None, None))

    def dcd(self, flags=0, fetch=True, samples=None):
        T = int(samples) if samples is not None else self.T
        ticks = T // 192
        sums = np.empty((self.C, ticks, 2, 6), dtype=np.float32) if fetch else None
        n = C.c_uint32(0)
        self._chk(self.lib.m17hip_dcd(self.h, C.c_uint32(self.C), C.c_uint32(T), C.c_uint32(flags), _ptr(sums), C.byref(n)))
        assert n.value == ticks
        return sums

    def viterbi(self, soft, kind):
        IN, OUT = VITERBI_SHAPES[kind]
        s = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1, IN)
        n = s.shape[0]
        bits = np.empty((n, OUT), dtype=np.uint8)
        cost = np.empty(n, dtype=np.int32)
        self._chk(self.lib.m17hip_viterbi(self.h, _ptr(s), C.c_uint32(n), C.c_int(kind), _ptr(bits), _ptr(cost)))
        return bits, cost

    def slice_llr(self, sym):
        s = np.ascontiguousarray(sym, dtype=np.float32)
        if s.ndim == 1:
            s = s[None, :]
        rows, n = s.shape
        llr = np.empty((rows, n, 2), dtype=np.int8)
        evm = np.empty((rows, n), dtype=np.float32)
        self._chk(self.lib.m17hip_slice_llr(self.h, _ptr(s), C.c_uint32(rows), C.c_uint32(n), _ptr(llr), _ptr(evm)))
        return llr, evm

    def decode_frames(self, llr368, sync_type, state=None, lich=None, lsf=None, dep401=None, cost=None):
        l = np.ascontiguousarray(llr368, dtype=np.int8).reshape(-1, 368)
        n = l.shape[0]
        st = np.ascontiguousarray(sync_type, dtype=np.uint8)
        state = np.zeros(n, np.uint8) if state is None else np.ascontiguousarray(state, dtype=np.uint8).copy()
        lich = np.zeros(n, np.uint8) if lich is None else np.ascontiguousarray(lich, dtype=np.uint8).copy()
        lsf = np.zeros((n, 30), np.uint8) if lsf is None else np.ascontiguousarray(lsf, dtype=np.uint8).copy()
        dep401 = np.zeros(n, np.int8) if dep401 is None else np.ascontiguousarray(dep401, dtype=np.int8).copy()
        cost = np.zeros(n, np.int64) if cost is None else np.ascontiguousarray(cost, dtype=np.int64).copy()
        recs = np.zeros((n, 2), dtype=FRAME_REC)
        nrec = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.m17hip_decode_frames(self.h, _ptr(l), C.c_uint32(n), _ptr(st), _ptr(state), _ptr(lich), _ptr(lsf), _ptr(dep401),
                                                _ptr(cost), _ptr(recs), _ptr(nrec)))
        return recs, nrec, state, lich, lsf, dep401, cost

    def decode_sequences(self, form, llr368, sync_type, rec_cap, state=None, lich=None, lsf=None, dep401=None, cost=None):
        """TEST HOOK (m17hip_decode_sequences): C sequences of F frames through the frame decoder in device form `form` (0 lane per channel, 1 wave
        per channel, 2 wave with a deferred-frame store + the kernels that settle and decode it).  llr368 [C][F][368] within [-7, 7], sync_type
        [C][F].  Returns (recs [C][rec_cap], nrec [C], overflow, state, lich, lsf, dep401, cost, cost_trace [C][F])."""
        l = np.ascontiguousarray(llr368, dtype=np.int8)
        if l.ndim != 3 or l.shape[2] != 368:
            raise TypeError("llr368 is [channels][frames][368]")
        n, F = l.shape[0], l.shape[1]
        st = np.ascontiguousarray(sync_type, dtype=np.uint8)
        if st.shape != (n, F):
            raise TypeError("sync_type is [channels][frames]")
        state = np.zeros(n, np.uint8) if state is None else np.ascontiguousarray(state, dtype=np.uint8).copy()
        lich = np.zeros(n, np.uint8) if lich is None else np.ascontiguousarray(lich, dtype=np.uint8).copy()
        lsf = np.zeros((n, 30), np.uint8) if lsf is None else np.ascontiguousarray(lsf, dtype=np.uint8).copy()
        dep401 = np.zeros(n, np.int8) if dep401 is None else np.ascontiguousarray(dep401, dtype=np.int8).copy()
        cost = np.zeros(n, np.int64) if cost is None else np.ascontiguousarray(cost, dtype=np.int64).copy()
        if state.shape != (n,) or lich.shape != (n,) or lsf.shape != (n, 30) or dep401.shape != (n,) or cost.shape != (n,):
            raise TypeError("the decoder state is one entry per channel")
        recs = np.zeros((n, max(int(rec_cap), 1)), dtype=FRAME_REC)
        nrec = np.zeros(n, dtype=np.uint32)
        ovf = C.c_uint32(0)
        trace = np.zeros((n, F), dtype=np.int32)
        self._chk(self.lib.m17hip_decode_sequences(self.h, C.c_int(form), _ptr(l), _ptr(st), C.c_uint32(n), C.c_uint32(F), C.c_uint32(rec_cap), _ptr(state),
                                                   _ptr(lich), _ptr(lsf), _ptr(dep401), _ptr(cost), _ptr(recs), _ptr(nrec), C.byref(ovf), _ptr(trace)))
        return recs, nrec, int(ovf.value), state, lich, lsf, dep401, cost, trace

    def set_fir_taps(self, taps149=None):
        """TEST HOOK (m17hip_set_fir_taps): the 149 taps every matched-filter form of this context reads from now on; None restores the RRC taps."""
        if taps149 is None:
            self._chk(self.lib.m17hip_set_fir_taps(self.h, None))
            return
        t = np.ascontiguousarray(taps149, dtype=np.float32)
        if t.shape != (149,):
            raise TypeError("taps149 is 149 floats")
        self._chk(self.lib.m17hip_set_fir_taps(self.h, _ptr(t)))

    def kalman_trace(self, z, dt, wrap, z0=0.0, order=3):
        """rows x n updates of the 2-state Kalman filter (kal_update, as the full-chain kernel runs it): state after each update."""
        zz = np.ascontiguousarray(z, dtype=np.float32)
        if zz.ndim == 1:
            zz = zz[None, :]
        dd = np.ascontiguousarray(np.broadcast_to(dt, zz.shape), dtype=np.uint32)
        out = np.empty(zz.shape + (6,), dtype=np.float32)
        self._chk(self.lib.m17hip_kalman_trace(self.h, _ptr(zz), _ptr(dd), C.c_uint32(zz.shape[0]), C.c_uint32(zz.shape[1]), C.c_int(wrap),
                                               C.c_float(z0), C.c_int(order), _ptr(out)))
        return out

    # ---- the full chain ----------------------------------------------------------------------------------------------
    def set_kalman_order(self, order):
        """Evaluation order of the Kalman updates (bit set, include/m17hip.h); default 3."""
        self._chk(self.lib.m17hip_set_kalman_order(self.h, C.c_int(order)))

    def set_channel_base(self, base):
        """Global id of this context's channel 0: frame records carry channel = base + local index."""
        self._chk(self.lib.m17hip_set_channel_base(self.h, C.c_uint32(base)))

    def gather_frames(self, comm, root=0, capacity=None):
        """Collective: the records of the last run of every rank, gathered to `root` over RCCL in rank (= channel) order.
        Returns (records or None off the root, counts per rank)."""
        counts = np.zeros(comm.nranks, dtype=np.uint64)
        total = C.c_uint64(0)
        is_root = comm.rank == root
        if capacity is None:
            capacity = comm.nranks * self.max_channels * (2 * (self.max_samples // 1920 + 2) + 4) if is_root else 0
        recs = np.empty(capacity, dtype=FRAME_REC) if is_root else None
        self._chk(self.lib.m17hip_gather_frames(self.h, comm.h, C.c_int(root), _ptr(recs), C.c_uint64(capacity), _ptr(counts), C.byref(total)))
        return (recs[: total.value] if is_root else None), counts

    def gather_frames_device(self, comm, dev_ptr, capacity, root=0):
        """Collective: like gather_frames, the root's copy written to device memory at dev_ptr.  Returns (total, counts per rank)."""
        counts = np.zeros(comm.nranks, dtype=np.uint64)
        total = C.c_uint64(0)
        self._chk(self.lib.m17hip_gather_frames_device(self.h, comm.h, C.c_int(root), C.c_void_p(int(dev_ptr)), C.c_uint64(capacity), _ptr(counts),
                                                       C.byref(total)))
        return total.value, counts

    def reset(self):
        self._chk(self.lib.m17hip_demod_reset(self.h))

    def reset_channels(self, indices):
        """Fresh demodulators for the listed channels only (local indices, duplicates allowed), from the start of the NEXT run queued (run(), or
        the front() that begins it); every other channel goes on.  Between runs whose lengths are multiples of 192 samples, and not between
        front() and run() (m17hip_demod_reset_channels).  Their IQ feeds (upload_iq*) start over with the IQ blocks uploaded after this call."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32).reshape(-1))
        self._chk(self.lib.m17hip_demod_reset_channels(self.h, _ptr(idx) if idx.size else None, C.c_uint32(idx.size)))

    def set_channel_polarity(self, invert):
        """Per-channel input polarity: `invert` is an array-like of 0 / 1 for local channels 0 .. len - 1 (later entries keep their value), or None
        to clear the table.  A channel's effective polarity in a call is its entry XOR the call's FLAG_INVERT.  Changing the entry of a channel
        that has run restarts it as reset_channels does, under that call's rule (m17hip_set_channel_polarity)."""
        if invert is None:
            self._chk(self.lib.m17hip_set_channel_polarity(self.h, None, C.c_uint32(0)))
            return
        a = np.asarray(invert).reshape(-1)
        if a.size == 0 or not np.all((a == 0) | (a == 1)):   # (an empty table is not "clear": that is None)
            self._chk(-1)
        tab = np.ascontiguousarray(a.astype(np.uint8))
        self._chk(self.lib.m17hip_set_channel_polarity(self.h, _ptr(tab), C.c_uint32(tab.size)))

    def run(self, flags=0, channels=None, samples=None):
        self._fed_channels = None
        if getattr(self, "_scan_pending", False):   # (wide_scan: a slot assigned in the block starts a new transmission on a demodulator fed zeros)
            self._scan_pending = False
            try:
                assigned = self.wide_scan_fetch()[3]
            except M17HipError as e:
                if "error -4" not in str(e):   # (M17HIP_ESTATE: a call since wide_scan has turned the scan off — every squelch, spectrum and configuration call does)
                    raise
                self._scan, assigned = False, []
            if assigned:
                self.reset_channels(assigned)
        self._chk(self.lib.m17hip_demod_run(self.h, C.c_uint32(channels or self.C), C.c_uint32(samples or self.T), C.c_uint32(flags)))

    def frames_select(self, back):
        """Which run's records frames_count / frames / frames_compact_device / gather_frames name: 0 = the latest run (every run() selects it
        again), 1 = the run before it (a live feed collects run k after it has queued run k + 1)."""
        self._chk(self.lib.m17hip_frames_select(self.h, C.c_uint32(back)))

    def frames_count(self):
        n = C.c_uint64(0)
        self._chk(self.lib.m17hip_frames_count(self.h, C.byref(n)))
        return n.value

    def frames(self):
        """Records of the last run, ordered by (channel, seq).  One compaction and one synchronisation when the guessed capacity (the
        previous fetch's count plus a margin) suffices; M17HIP_ETRUNC reports the real count and the fetch is repeated once."""
        cap = max(1024, getattr(self, "_last_frames", 0) * 5 // 4 + 64)
        while True:
            recs = np.zeros(cap, dtype=FRAME_REC)
            got = C.c_uint64(0)
            code = self.lib.m17hip_frames_fetch(self.h, _ptr(recs), C.c_uint64(recs.size), C.byref(got))
            if code == ETRUNC and got.value > cap:
                cap = int(got.value)
                continue
            self._chk(code)
            self._last_frames = int(got.value)
            return recs[: got.value]

    def frames_compact_device(self, dev_ptr, capacity):
        n = C.c_uint64(0)
        self._chk(self.lib.m17hip_frames_compact_device(self.h, C.c_void_p(int(dev_ptr)), C.c_uint64(capacity), C.byref(n)))
        return n.value

    def diag(self, channels=None):
        n = channels or self.C
        d = np.zeros(n, dtype=DIAG)
        self._chk(self.lib.m17hip_diag_fetch(self.h, _ptr(d), C.c_uint32(n)))
        return d

    def diag_log(self, channels=None, capacity=None):
        """Every diagnostic callback of the last run per channel (enable with tune(9, room) before the run): list of DIAG arrays."""
        n = channels or self.C
        cap = capacity or (self.T // 384 + 2)
        log = np.zeros((n, cap), dtype=DIAG)
        counts = np.zeros(n, dtype=np.uint32)
        self._chk(self.lib.m17hip_diag_log_fetch(self.h, _ptr(log), _ptr(counts), C.c_uint32(n), C.c_uint32(cap)))
        return [log[c, : counts[c]] for c in range(n)]

    def lsf_info(self, lsf30):
        """Callsigns, type field and CRC status of a batch of 30-byte link setup frames."""
        a = np.ascontiguousarray(lsf30, dtype=np.uint8).reshape(-1, 30)
        out = np.zeros(a.shape[0], dtype=LSF_INFO)
        self._chk(self.lib.m17hip_lsf_info(self.h, _ptr(a), C.c_uint32(a.shape[0]), _ptr(out)))
        return out

    def bert_stats(self, channels=None):
        """PRBS9 bit / error counts per channel over the BERT frames since reset (enable with tune(6, 1) before the runs)."""
        n = channels or self.C
        st = np.zeros(n, dtype=BERT_STAT)
        self._chk(self.lib.m17hip_bert_stats(self.h, _ptr(st), C.c_uint32(n)))
        return st

    def sweep_stats(self, n_points, channels=None):
        """One CHAN_STAT_DTYPE word per channel: the PRBS9 counts of bert_stats and the `evm` of diag, with channel = channel base + index and
        point = channel % n_points (m17hip_sweep_stats).  A deferred-EVM overflow (M17HIP_EOVERFLOW) is not raised: those words carry flags
        bit 0 cleared."""
        n = channels or self.C
        w = np.zeros(n, dtype=CHAN_STAT_DTYPE)
        code = self.lib.m17hip_sweep_stats(self.h, C.c_uint32(n_points), _ptr(w), C.c_uint32(n))
        if code != EOVERFLOW:
            self._chk(code)
        return w

    def gather_sweep_stats(self, comm, words, root=0, capacity=None):
        """Collective: every rank's sweep words (any number per rank) gathered to `root` in rank order (m17hip_gather_sweep_stats).  Returns
        (words or None off the root, counts per rank).  `capacity` (root): room for the gathered words, by default nranks x max(len(words),
        max_channels); a gathered set that does not fit raises."""
        w = np.ascontiguousarray(np.asarray(words, dtype=CHAN_STAT_DTYPE).reshape(-1))
        counts = np.zeros(comm.nranks, dtype=np.uint64)
        total = C.c_uint64(0)
        is_root = comm.rank == root
        if capacity is None:
            capacity = comm.nranks * max(w.size, self.max_channels) if is_root else 0
        out = np.zeros(capacity, dtype=CHAN_STAT_DTYPE) if is_root else None
        self._chk(self.lib.m17hip_gather_sweep_stats(self.h, comm.h, C.c_int(root), _ptr(w), C.c_uint64(w.size), _ptr(out), C.c_uint64(capacity),
                                                     _ptr(counts), C.byref(total)))
        return (out[: total.value] if is_root else None), counts

    def packets(self, capacity=4096):
        """Packets the last run completed, ordered by (channel, seq) (enable with tune(7, room) before the runs)."""
        out = np.zeros(capacity, dtype=PACKET_REC)
        n = C.c_uint32(0)
        self._chk(self.lib.m17hip_packets_fetch(self.h, _ptr(out), C.c_uint32(capacity), C.byref(n)))
        return out[: min(n.value, capacity)]

    def packets_feed(self, recs2d, counts):
        """Run the packet consumer over caller-supplied frame records [channels][pitch] (counts[c] used per row)."""
        r = np.ascontiguousarray(recs2d, dtype=FRAME_REC)
        n = np.ascontiguousarray(counts, dtype=np.uint32)
        self._chk(self.lib.m17hip_packets_feed(self.h, _ptr(r), _ptr(n), C.c_uint32(r.shape[0]), C.c_uint32(r.shape[1])))

    # ---- the voice consumer (tune(34, room) before the runs) ---------------------------------------------------------
    def voice(self, slots=None, channels=None):
        """The codec2 payload planes of the selected run: (audio uint8[C, n, 16], marks uint8[C, n], counts uint32[C]).  counts[c] stream
        records of channel c, in arrival order; marks: MARK_BLANK / MARK_EOS / MARK_FIRST / MARK_GAP.  n = `slots`, by default the largest
        count (cut at the room).  More records than the room (M17HIP_EOVERFLOW) or than `slots` (M17HIP_ETRUNC) raise; the C entry point
        (m17hip_voice_fetch) returns the rows as far as they go."""
        C_ = channels or getattr(self, "_fed_channels", None) or self.C
        counts = np.zeros(C_, dtype=np.uint32)
        if slots is None:   # the counts first: the planes are then fetched as wide as they are used
            code = self.lib.m17hip_voice_fetch(self.h, None, None, _ptr(counts), C.c_uint32(C_), C.c_uint32(0))
            if code != ETRUNC:
                self._chk(code)
            slots = int(counts.max()) if C_ else 0
        n = int(slots)
        audio = np.zeros((C_, n, 16), dtype=np.uint8)
        marks = np.zeros((C_, n), dtype=np.uint8)
        self._chk(self.lib.m17hip_voice_fetch(self.h, _ptr(audio) if n else None, _ptr(marks) if n else None, _ptr(counts), C.c_uint32(C_), C.c_uint32(n)))
        return audio, marks, counts

    def voice_device(self):
        """Raw DEVICE pointers of the selected run's planes, (audio, marks, counts, pitch_slots): audio[max_channels][pitch_slots][16] uint8,
        marks[max_channels][pitch_slots] uint8, counts[max_channels] uint32 — valid until the run after the next is queued
        (m17hip_voice_device); the payload work of that run is complete when this returns."""
        a, m, n, pitch = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        self._chk(self.lib.m17hip_voice_device(self.h, C.byref(a), C.byref(m), C.byref(n), C.byref(pitch)))
        return a.value or 0, m.value or 0, n.value or 0, pitch.value

    def calls(self, capacity=4096):
        """Calls the selected run closed, ordered by (channel, seq): a CALL_REC array (m17hip_calls_fetch)."""
        out = np.zeros(capacity, dtype=CALL_REC)
        n = C.c_uint32(0)
        self._chk(self.lib.m17hip_calls_fetch(self.h, _ptr(out) if capacity else None, C.c_uint32(capacity), C.byref(n)))
        return out[: min(n.value, capacity)]

    def voice_feed(self, recs2d, counts):
        """Run the voice consumer over caller-supplied frame records [channels][pitch] (counts[c] used per row); voice() and calls() then
        return what it made of them."""
        r = np.ascontiguousarray(recs2d, dtype=FRAME_REC)
        n = np.ascontiguousarray(counts, dtype=np.uint32)
        self._chk(self.lib.m17hip_voice_feed(self.h, _ptr(r), _ptr(n), C.c_uint32(r.shape[0]), C.c_uint32(r.shape[1])))
        self._fed_channels = r.shape[0]   # (what voice() names by default until the next run)

    def replay_drops(self):
        """Times a channel left the limit-filter replay since the last reset (m17hip_replay_drops)."""
        n = C.c_uint64(0)
        self._chk(self.lib.m17hip_replay_drops(self.h, C.byref(n)))
        return int(n.value)

    def tune(self, key, value):
        self._chk(self.lib.m17hip_tune(self.h, C.c_int(key), C.c_int64(value)))

    def debug_counters(self, max_waves=4096):
        buf = np.zeros((max_waves, 40), dtype=np.uint64)   # (csrc/m17_state.hpp DBG_SLOTS)
        n = C.c_uint32(0)
        self._chk(self.lib.m17hip_debug_counters(self.h, _ptr(buf), C.c_uint32(max_waves), C.byref(n)))
        return buf[: n.value]

    # ---- measurement ---------------------------------------------------------------------------------------------------
    def timing(self, on=True):
        self._chk(self.lib.m17hip_timing_enable(self.h, C.c_int(1 if on else 0)))

    def timing_reset(self):
        self._chk(self.lib.m17hip_timing_reset(self.h))

    def timing_get(self, kernel):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._chk(self.lib.m17hip_timing_get(self.h, C.c_int(KERNELS[kernel]), C.byref(ms), C.byref(n)))
        return ms.value, n.value
