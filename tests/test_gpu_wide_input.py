"""GPU tests of wideband IQ input (ABI 609, include/m17hip.h: m17hip_wide_config, m17hip_wide_channels, m17hip_upload_wide and friends): tune_kernel mixes,
low-pass filters, decimates and discriminates into the float input slab, and from there on the stream is a float stream.  Every comparison is exact: the
floats (m17hip_download_f32) as uint32 words against the HOST form of the same arithmetic (tests/cxx/wide_oracle.cpp: detail/core.h under the host compiler)
— NaN-ness where that is a NaN — and records, m17_diag and the diagnostic log byte for byte against the float oracle (tests/cxx/f32_oracle.cpp) stepped on
the host form's floats.  What the host form itself is worth is asserted without a GPU in tests/test_wide_input.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
THREADS = 16
INV = m17hip.FLAG_INVERT
INT_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock")
FMTS = {"i16": wl.IQ_I16, "f32": wl.IQ_F32, "u8": wl.IQ_U8}
GAINS = (1.0, 5.0 / 3.0)
SB = {wl.IQ_I16: 4, wl.IQ_F32: 8, wl.IQ_U8: 2}   # bytes per complex sample
INT32_MIN = -(1 << 31)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_words(got, exp, what):
    """Equal words; where the host form gives a NaN, a NaN (payload unspecified)."""
    nan = np.isnan(exp)
    assert np.isnan(got[nan]).all(), (what, "NaN expected")
    bad = np.argwhere((_u32(got) != _u32(exp)) & ~nan)
    assert bad.size == 0, (what, bad[:8].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _dev(a):
    """The array on the device, COMPLETE when this returns (the context's streams do not wait for torch's)."""
    import torch
    t = torch.from_numpy(np.array(a)).cuda()   # (a writable copy: the fixtures are read-only)
    torch.cuda.synchronize()
    return t


def _raw(ctx, name, ptr, Cn, T, pitch, gain=1.0):
    return getattr(ctx.lib, name)(ctx.h, C.c_void_p(ptr), C.c_float(gain), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(pitch))


def _config(ctx, S, R, fmt, taps):
    t = np.ascontiguousarray(taps, dtype=np.float32)
    return ctx.lib.m17hip_wide_config(ctx.h, C.c_uint32(S), C.c_uint32(R), C.c_int(fmt), ol._p(t), C.c_uint32(t.size))


def _spice(z, rng):
    """Components up to +-1e9, denormals of magnitude 1e-40 and +-0 sprinkled over every row of complex64 z (as the ABI 608 test does)."""
    v = z.view(np.float32).reshape(z.shape[0], -1)
    n = v.shape[1]
    for row in v:
        k = max(1, n // 11)
        row[rng.integers(0, n, k)] = (10.0 ** rng.uniform(0, 9, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
        row[rng.integers(0, n, k)] = np.float32(1e-40) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), k)
        row[rng.integers(0, n, k)] = rng.choice(np.array([-0.0, 0.0], dtype=np.float32), k)
        row[2 * rng.integers(1, n // 2, 3) + 1] = 0.0
    return z


# ---- 1: one hop ----------------------------------------------------------------------------------------------------------------------------------
# a tile is 255 outputs (one wave, four filter sums per lane): its edges +- 1, two tiles +- 1, and the sizes every block kernel is asked
HOP_TS = (1, 2, 3, 63, 64, 65, 254, 255, 256, 257, 509, 510, 511, 1025)
HOP_RS = (1, 2, 5, 16)
HOP_S, HOP_C = 3, 65
HOP_CN = (1, 3, 65)
BAD_SRC = 1   # the float source that holds infinities and NaNs: they stay in the channels that listen to it.  Source 2 is heard by nobody.
HOP_SRC = np.array([c % 2 for c in range(HOP_C)], dtype=np.uint32)   # 33 channels on source 0, 32 on source 1


def _hop_ls(R):
    return sorted({1, R, 4 * R + 1, min(32 * R + 1, 513)})


def _hop_pitch(R):
    return max(HOP_TS) * R + 3   # odd: row 1 of int16 / uint8 and no float row but 0 and 2 begins 16-byte aligned (a sample is aligned to its own size, no more)


@pytest.fixture(scope="module")
def hop_words():
    rng = np.random.default_rng(609)
    fcw = rng.integers(INT32_MIN, 1 << 31, HOP_C).astype(np.int64)
    fcw[:6] = (0, 1 << 30, -(1 << 30), INT32_MIN, 1, -1)
    return fcw


def _hop_data(fmt, R, rng):
    P = _hop_pitch(R)
    if fmt == wl.IQ_I16:
        x = rng.integers(-32768, 32768, size=(HOP_S, P, 2)).astype(np.int16)
        x[:, 5] = (-32768, 32767)
        x[:, 9] = 0
    elif fmt == wl.IQ_U8:
        x = rng.integers(0, 256, size=(HOP_S, P, 2)).astype(np.uint8)
        x[:, 5] = (0, 255)
    else:
        x = (12000.0 * (rng.standard_normal((HOP_S, P)) + 1j * rng.standard_normal((HOP_S, P)))).astype(np.complex64)
        x[:, 8:10] = 0
        x = _spice(x, rng)
        v = x[BAD_SRC].view(np.float32)
        for k, val in zip(rng.choice(np.arange(40, 2 * P, 97), 9, replace=False), [np.inf, -np.inf, np.nan] * 3):
            v[k] = val
        v[6] = np.inf
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("R", HOP_RS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_tuner_one_hop(hop_words, fmt, R):
    """Host and device sources, pitch > samples * R with aligned and unaligned rows, both gains, every tile edge, every tap count, 1 and 3 sources, 1, 3 and
    65 channels (several on one source, one source unheard; frequency words 0, +-2^30, INT32_MIN and random ones): the host form's words.  The float rows
    hold values up to 1e9, denormals and zeroes; one source infinities and NaNs, which stay in the channels that listen to it."""
    f = FMTS[fmt]
    rng = np.random.default_rng(6090 + 16 * f + R)
    host = _hop_data(f, R, rng)
    dev = _dev(host)
    P, Tmax = _hop_pitch(R), max(HOP_TS)
    fcw = hop_words
    ctx = m17hip.Context(HOP_C, Tmax)
    try:
        for li, L in enumerate(_hop_ls(R)):
            taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
            S = 1 if li == 1 else HOP_S   # (one pass with a single source: every channel listens to source 0, three channels at the most)
            src = np.zeros(HOP_C, dtype=np.uint32) if S == 1 else HOP_SRC
            chans = 3 if S == 1 else HOP_C
            exp = {g: np.stack([wl.tune(host[src[c]][: Tmax * R], taps, R, int(fcw[c]), g) for c in range(chans)]) for g in GAINS}
            if f == wl.IQ_F32 and S > 1 and L >= R:   # (sample 3 of the bad source is infinite: inside the first output's window)
                e = exp[1.0]
                assert np.isnan(e[BAD_SRC::2]).any() and np.isfinite(e[0::2]).all()
            assert _config(ctx, S, R, f, taps) == 0
            ctx.wide_channels(src, fcw)
            for ti, T in enumerate(HOP_TS):
                Cn = 65 if T == Tmax else HOP_CN[ti % 3]
                Cn = min(Cn, chans)
                for k, way in enumerate(("host", "device")):
                    gain = GAINS[(ti + k) & 1]
                    ctx.reset()   # (a fresh feed: histories, count and carries are zero)
                    name, ptr = ("m17hip_upload_wide", host.ctypes.data) if way == "host" else ("m17hip_upload_wide_device", dev.data_ptr())
                    assert _raw(ctx, name, ptr, Cn, T, P, gain) == 0
                    ctx.C, ctx.T = Cn, T
                    assert ctx.input_format()[0] == m17hip.FORMAT_F32
                    _assert_words(ctx.download_f32(), exp[gain][:Cn, :T], (fmt, R, L, S, Cn, T, gain, way))
    finally:
        ctx.close()


# ---- 2: the feed ---------------------------------------------------------------------------------------------------------------------------------
FEED_R, FEED_L, FEED_S, FEED_C = 5, 81, 2, 5
FEED_LENS = (1, 2, 255, 1024, 3, 700)   # outputs per block; behind the block of 3 the history of L - 1 = 80 samples still holds 65 of the block before it
FEED_CUTS = np.cumsum((0,) + FEED_LENS).tolist()
FEED_T = FEED_CUTS[-1]
FEED_SRC = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
FEED_FCW = np.array([m17hip.wide_fcw(f, FEED_R) for f in (12500.0, -75000.0, 0.0, 101000.0, -3000.0)], dtype=np.int64)
FEED_GAIN = 1.25


@pytest.fixture(scope="module")
def feed_case():
    """Two sources in all three formats (the float one holds the int16 one's values) and the one-block result of five channels on them."""
    rng = np.random.default_rng(6091)
    W = FEED_T * FEED_R
    xi = rng.integers(-20000, 20001, size=(FEED_S, W, 2)).astype(np.int16)
    xf = (xi[..., 0].astype(np.float32) + 1j * xi[..., 1].astype(np.float32)).astype(np.complex64)
    xu = rng.integers(0, 256, size=(FEED_S, W, 2)).astype(np.uint8)
    taps = (rng.standard_normal(FEED_L) / 9.0).astype(np.float32)
    data = {wl.IQ_I16: xi, wl.IQ_F32: xf, wl.IQ_U8: xu}
    whole = {f: wl.tune_channels(x, FEED_SRC, FEED_FCW, taps, FEED_R, FEED_GAIN) for f, x in data.items()}
    assert np.array_equal(_u32(whole[wl.IQ_I16]), _u32(whole[wl.IQ_F32]))
    for a in list(data.values()) + list(whole.values()):
        a.setflags(write=False)
    return data, taps, whole


@pytest.mark.parametrize("source", ["pinned_i16", "device_f32", "device_u8"])
def test_blocks_continue_one_another_across_the_main_and_the_copy_stream(feed_case, source):
    """Blocks cut at 1, 2, 255, 1024, 3 and the rest, in place on the main stream and staged on the copy stream by turns: each finds the sources' histories
    and the channels' carries the block before it left, whichever stream that ran on — the concatenation is the one-block result."""
    import torch
    data, taps, whole = feed_case
    f = {"pinned_i16": wl.IQ_I16, "device_f32": wl.IQ_F32, "device_u8": wl.IQ_U8}[source]
    dev = _dev(data[f])
    pin = torch.from_numpy(np.array(data[f])).pin_memory()
    sb, W = SB[f], FEED_T * FEED_R
    ctx = m17hip.Context(FEED_C, max(FEED_LENS))
    try:
        ctx.wide_config(FEED_S, FEED_R, f, taps)
        ctx.wide_channels(FEED_SRC, FEED_FCW)
        ctx.reset()
        how = ["in_place", "staged_run", "in_place", "staged_run", "staged_run", "in_place"]
        for (a, b), h in zip(zip(FEED_CUTS[:-1], FEED_CUTS[1:]), how):
            off = a * FEED_R * sb
            if h == "in_place":
                ctx.upload_wide_device(dev.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
            else:
                if source.startswith("device"):
                    ctx.upload_wide_device_async(dev.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
                else:
                    ctx.upload_wide_async(pin.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
                ctx.run(channels=FEED_C, samples=b - a)
            _assert_words(ctx.download_f32(), whole[f][:, a:b], (source, h, a, b))
        ctx.upload_wait()
    finally:
        ctx.close()


def test_host_blocks_continue_one_another(feed_case):
    """The host form of the call (the raw block goes through the context's own buffer, which grows), numpy arrays through Context.upload_wide."""
    data, taps, whole = feed_case
    for f in (wl.IQ_U8, wl.IQ_I16, wl.IQ_F32):
        ctx = m17hip.Context(FEED_C, max(FEED_LENS))
        try:
            ctx.wide_config(FEED_S, FEED_R, f, taps)
            ctx.wide_channels(FEED_SRC, FEED_FCW)
            parts = []
            for a, b in zip(FEED_CUTS[:-1], FEED_CUTS[1:]):
                ctx.upload_wide(data[f][:, a * FEED_R: b * FEED_R], gain=FEED_GAIN)
                parts.append(ctx.download_f32())
            _assert_words(np.concatenate(parts, axis=1), whole[f], f)
        finally:
            ctx.close()


# ---- 3: table changes ------------------------------------------------------------------------------------------------------------------------------
def _feeds(data, taps, src, fcw):
    """One host-form tuner per channel, fed block by block (wide_lib.Feeds at this module's decimation and gain)."""
    return wl.Feeds(data, taps, src, fcw, FEED_R, FEED_GAIN)


def test_table_changes_resets_and_what_a_staged_block_keeps(feed_case):
    data, taps, whole = feed_case
    f = wl.IQ_I16
    x = data[f]
    dev = _dev(x)
    sb, W = SB[f], FEED_T * FEED_R
    T = 192
    ctx = m17hip.Context(FEED_C, T)
    ref = _feeds(x, taps, FEED_SRC, FEED_FCW)
    try:
        ctx.wide_config(FEED_S, FEED_R, f, taps)
        ctx.wide_channels(FEED_SRC, FEED_FCW)
        ctx.reset()

        def up(k, staged=False):
            getattr(ctx, "upload_wide_device_async" if staged else "upload_wide_device")(dev.data_ptr() + k * T * FEED_R * sb, FEED_C, T, W, FEED_GAIN)

        up(0)
        _assert_words(ctx.download_f32(), ref.block(0, T), "block 0")
        # a retune between blocks: channel 0 to another offset, channel 1 to the other source; only the first two entries are given, the others keep theirs
        ctx.wide_channels([0, 0], [m17hip.wide_fcw(-40000.0, FEED_R), FEED_FCW[1]])
        ref.src[1], ref.fcw[0] = 0, m17hip.wide_fcw(-40000.0, FEED_R)
        up(1)
        e1 = ref.block(T, 2 * T)
        assert not np.array_equal(_u32(e1[:2]), _u32(whole[f][:2, T:2 * T])) and np.array_equal(_u32(e1[2:]), _u32(whole[f][2:, T:2 * T]))
        _assert_words(ctx.download_f32(), e1, "block 1, retuned")
        # a staged block keeps the table it was tuned with: the change behind it applies from the block after
        up(2, staged=True)
        ctx.wide_channels([1], [0])
        e2 = ref.block(2 * T, 3 * T)
        ref.src[0], ref.fcw[0] = 1, 0
        ctx.run(channels=FEED_C, samples=T)
        _assert_words(ctx.download_f32(), e2, "block 2, staged before the change")
        up(3)
        _assert_words(ctx.download_f32(), ref.block(3 * T, 4 * T), "block 3, after the change")
        # reset_channels: the listed channels' carries are zero at once (the stream stands at 192 samples: on the tick grid); nothing else changes
        ctx.reset_channels([1, 3])
        for c in (1, 3):
            ref.carry[c] = np.zeros(2, dtype=np.float32)
        up(4)
        e4 = ref.block(4 * T, 5 * T)
        assert (e4[[1, 3], 0] == 0).all() and (e4[[0, 2, 4], 0] != 0).all()
        _assert_words(ctx.download_f32(), e4, "block 4, two carries zeroed")
        # invalid tables change nothing
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.array([0, FEED_S], dtype=np.uint32)), ol._p(np.zeros(2, dtype=np.int32)), C.c_uint32(2)) == EINVAL
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.zeros(FEED_C + 1, dtype=np.uint32)), ol._p(np.zeros(FEED_C + 1, dtype=np.int32)), C.c_uint32(FEED_C + 1)) == EINVAL
        assert ctx.lib.m17hip_wide_channels(ctx.h, None, None, C.c_uint32(1)) == EINVAL
        assert ctx.lib.m17hip_wide_channels(ctx.h, None, None, C.c_uint32(0)) == 0
        up(5)
        _assert_words(ctx.download_f32(), ref.block(5 * T, 6 * T), "block 5, after refused tables")
        # demod_reset: count, histories and carries start over — a fresh host form on the same table
        ctx.reset()
        up(6)
        fresh = _feeds(x[:, 6 * T * FEED_R:], taps, ref.src, ref.fcw)
        e6 = fresh.block(0, T)
        assert not np.array_equal(_u32(e6), _u32(ref.block(6 * T, 7 * T)))
        _assert_words(ctx.download_f32(), e6, "block 6, after reset")
        # wide_config again starts the sources over and leaves the carries
        assert _config(ctx, FEED_S, FEED_R, f, taps) == 0
        up(7)
        again = _feeds(x[:, 7 * T * FEED_R:], taps, ref.src, ref.fcw)
        again.carry = [c.copy() for c in fresh.carry]
        _assert_words(ctx.download_f32(), again.block(0, T), "block 7, after a second wide_config")
    finally:
        ctx.close()


# ---- 4: the full chain ---------------------------------------------------------------------------------------------------------------------------
CH_R = 5
CH_OFFSETS = (-75000.0, 12500.0, 25000.0)
CH_KINDS = (1, 2, 4)
CH_C = 6   # channels 0..2: the three transmissions on source 0; 3..5: the same on source 1 — the spectrum flipped — at the mirrored offsets, inverted


class Expect:
    """The float oracle over whole streams y[C][T] (channel c under invert[c]): records and log entries of the run that covers samples [b0, b1) of the
    context's stream, and m17_diag at the end of the stream."""

    def __init__(self, y, invert=None):
        self.C, self.T = y.shape
        inv = np.zeros(self.C, dtype=np.uint8) if invert is None else np.asarray(invert, dtype=np.uint8)
        r, n, d, lg, ln = fl.demod_batch(np.ascontiguousarray(y), invert=inv, threads=THREADS, logs=True)
        self.recs = [r[c, : n[c]].copy() for c in range(self.C)]
        for c in range(self.C):
            self.recs[c]["channel"] = c
        self.logs = [lg[c, : ln[c]].copy() for c in range(self.C)]
        self.diags = d

    def run(self, b0, b1):
        rows, logs = [], []
        for c in range(self.C):
            r = self.recs[c]
            rows.append(r[(r["sample_pos"] >= b0) & (r["sample_pos"] < b1)].copy())
            lg = self.logs[c]
            pos = lg["pad"][:, 0].astype(np.int64) | (lg["pad"][:, 1].astype(np.int64) << 32)
            logs.append(lg[(pos >= b0) & (pos < b1)])
        return rows, logs


def _check(ctx, rows, logs, what, cap, diags=None, got=None):
    Cn = len(rows)
    got = ctx.frames().copy() if got is None else got
    e = np.concatenate(rows)
    if got.tobytes() != e.tobytes():
        bad = [c for c in range(Cn) if got[got["channel"] == c].tobytes() != rows[c].tobytes()]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {e.size} expected), channels {bad[:24]}")
    if logs is not None:
        glog = ctx.diag_log(Cn, capacity=cap)
        for c in range(Cn):
            assert glog[c].tobytes() == logs[c].tobytes(), (what, "diagnostic log", c, glog[c].size, logs[c].size)
    if diags is not None:
        d = ctx.diag(Cn)
        for fld in INT_FIELDS:
            assert np.array_equal(d[fld], diags[fld]), (what, fld, np.flatnonzero(d[fld] != diags[fld])[:16].tolist())
        for fld in FLOAT_FIELDS:
            assert np.array_equal(d[fld], diags[fld], equal_nan=True), (what, fld)


@pytest.fixture(scope="module")
def chain_case():
    """The int16 wideband of tests/test_wide_input.py at R = 5 (three FM transmissions, one 12.5 kHz from its neighbour) as source 0 and its conjugate as
    source 1; six channels, the last three inverted; the host form's floats and the float oracle's verdict on them."""
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in CH_KINDS]
    x0 = wl.wideband(bb, CH_OFFSETS, CH_R, amplitude=6000.0, sigma=300.0, seed=1, fmt=wl.IQ_I16)
    x = np.stack([x0, x0 * np.array([1, -1], dtype=np.int16)])
    src = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint32)
    fcw = np.array([m17hip.wide_fcw(f, CH_R) for f in CH_OFFSETS] + [m17hip.wide_fcw(-f, CH_R) for f in CH_OFFSETS], dtype=np.int64)
    pol = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8)
    taps = m17hip.wide_default_taps(CH_R)
    y = wl.tune_channels(x, src, fcw, taps, CH_R, 1.0)
    exp = Expect(y, invert=pol)
    good = [r[(r["cost"] < 30) & (r["frame_type"] != 1)] for r in exp.recs]
    assert all(g.size >= 7 for g in good), "every channel yields its transmission's frames"
    for c in range(3):
        assert good[c]["payload"].tobytes() == good[c + 3]["payload"].tobytes()
    for a in (x, y):
        a.setflags(write=False)
    return x, src, fcw, pol, y, exp


@pytest.mark.parametrize("src_kind", ["host", "tensor"])
def test_full_chain_in_one_run(chain_case, src_kind):
    x, src, fcw, pol, y, exp = chain_case
    T = y.shape[1]
    cap = T // 384 + 2
    ctx = m17hip.Context(CH_C, T)
    try:
        ctx.tune(9, cap)
        ctx.wide_config(2, CH_R)   # (int16, the default taps)
        ctx.wide_channels(src, fcw)
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_wide(x if src_kind == "host" else _dev(x))
        _assert_words(ctx.download_f32(), y, src_kind)
        ctx.run()
        rows, logs = exp.run(0, T)
        _check(ctx, rows, logs, src_kind, cap, diags=exp.diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
def test_full_chain_pipelined_in_ragged_segments(chain_case, order):
    """A live feed: m17hip_upload_wide_device_async of segment k + 1, m17hip_demod_front, run — the tuner of the next segment on the copy stream beside the
    state-machine half of the current run; segments of ragged multiples of 192, mixed polarity."""
    x, src, fcw, pol, y, exp = chain_case
    T = y.shape[1]
    b = [0, 192, 192 * 27, 192 * 28, 192 * 75, 192 * 120, T]
    lens = [b1 - b0 for b0, b1 in zip(b[:-1], b[1:])]
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(CH_C, max(lens))
    try:
        ctx.wide_config(2, CH_R)
        ctx.wide_channels(src, fcw)
        ctx.set_channel_polarity(pol)
        ctx.reset()

        def stage(k):
            ctx.upload_wide_device_async(dev.data_ptr() + b[k] * CH_R * sb, CH_C, lens[k], W)

        stage(0)
        ctx.run(channels=CH_C, samples=lens[0])
        for k in range(len(lens)):
            more = k + 1 < len(lens)
            if more:
                stage(k + 1)
                ctx.front(channels=CH_C, samples=lens[k + 1])
                if order == "run_then_fetch":
                    ctx.run(channels=CH_C, samples=lens[k + 1])
                    ctx.frames_select(1)
            got = ctx.frames().copy()
            ctx.frames_select(0)
            rows, _ = exp.run(b[k], b[k + 1])
            _check(ctx, rows, None, f"pipelined {order}, segment {k}", 0, diags=None if more else exp.diags, got=got)
            if more and order != "run_then_fetch":
                ctx.run(channels=CH_C, samples=lens[k + 1])
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


# ---- 5: state rules ------------------------------------------------------------------------------------------------------------------------------
NAMES = ("m17hip_upload_wide", "m17hip_upload_wide_async", "m17hip_upload_wide_device", "m17hip_upload_wide_device_async")


def test_state_rules_memory_and_timing(feed_case):
    import torch
    data, taps, whole = feed_case
    Cn, T, R, L = FEED_C, 960, FEED_R, FEED_L
    xi = np.ascontiguousarray(data[wl.IQ_I16][:, : T * R])
    dev, pin = _dev(xi), torch.from_numpy(xi.copy()).pin_memory()
    ptrs = dict(zip(NAMES, (xi.ctypes.data, pin.data_ptr(), dev.data_ptr(), dev.data_ptr())))
    si = np.zeros((Cn, T), dtype=np.int16)
    ctx = m17hip.Context(Cn + 2, T)
    maxC = Cn + 2
    try:
        assert ctx.iq_bytes() == 0
        for name in NAMES:   # before wide_config
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.zeros(1, dtype=np.uint32)), ol._p(np.zeros(1, dtype=np.int32)), C.c_uint32(1)) == ESTATE
        assert ctx.iq_bytes() == 0 and ctx.input_format() == (0, 0)
        # every refusal of wide_config
        one = np.ones(1, dtype=np.float32)
        for S, Rr, fm, tp, n in ((0, 5, 1, one, 1), (257, 5, 1, one, 1), (1, 0, 1, one, 1), (1, 17, 1, one, 1), (1, 5, 0, one, 1), (1, 5, 4, one, 1), (1, 5, 1, one, 0),
                                 (1, 5, 1, None, 1), (1, 5, 1, np.ones(1025, dtype=np.float32), 1025), (1, 5, 1, np.array([np.inf], dtype=np.float32), 1),
                                 (1, 5, 1, np.array([1.0, np.nan], dtype=np.float32), 2)):
            assert ctx.lib.m17hip_wide_config(ctx.h, C.c_uint32(S), C.c_uint32(Rr), C.c_int(fm), None if tp is None else ol._p(tp), C.c_uint32(n)) == EINVAL, (S, Rr, fm, n)
        assert ctx.iq_bytes() == 0
        assert ctx.lib.m17hip_wide_config(ctx.h, C.c_uint32(256), C.c_uint32(16), C.c_int(3), ol._p(np.ones(1024, dtype=np.float32)), C.c_uint32(1024)) == 0   # (the limits themselves)
        # on an int16 stream: refused, nothing changed
        ctx.upload(si)
        ctx.run()
        ctx.wide_config(FEED_S, R, wl.IQ_I16, taps)
        held = ctx.iq_bytes()
        assert held == maxC * 8 + L * 4 + 2 * FEED_S * (L - 1) * 8 + maxC * 8, "the carry; taps, two histories and the z of a launch"
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        assert ctx.input_format() == (m17hip.FORMAT_I16, 0) and ctx.iq_bytes() == held
        ctx.reset()   # frees the choice
        ctx.wide_channels(FEED_SRC, FEED_FCW)
        ctx.timing(True)
        ctx.upload_wide_device(dev.data_ptr(), Cn, T, T * R, FEED_GAIN)
        assert ctx.iq_bytes() == held + 2 * maxC * 4, "the device forms add one copy of the channel table"
        _assert_words(ctx.download_f32(), whole[wl.IQ_I16][:, :T], "device")
        ctx.reset()
        ctx.upload_wide(xi, gain=FEED_GAIN, channels=Cn)
        assert ctx.iq_bytes() == held + 2 * maxC * 4 + FEED_S * T * R * 4, "and the host forms the raw block"
        _assert_words(ctx.download_f32(), whole[wl.IQ_I16][:, :T], "host")
        ms, launches = ctx.timing_get("tune")
        assert launches == 2 and ms > 0, "one launch per block"
        assert ctx.timing_get("discriminate")[1] == 0
        ctx.timing(False)
        # the argument refusals, every way in
        for name in NAMES:
            p = ptrs[name]
            assert _raw(ctx, name, None, Cn, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, 0, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, 0, T * R) == EINVAL, name
            assert _raw(ctx, name, p, maxC + 1, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T + 1, (T + 1) * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T, T * R - 1) == EINVAL, name
            for bad_gain in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
                assert _raw(ctx, name, p, Cn, T, T * R, bad_gain) == EINVAL, (name, bad_gain)
        # m17hip_upload_iq goes on refusing format 3
        z = np.zeros((Cn, T, 2), dtype=np.uint8)
        assert ctx.lib.m17hip_upload_iq(ctx.h, ol._p(z), C.c_int(3), C.c_float(1.0), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(T)) == EINVAL
        # while a front end queued by m17hip_demod_front waits for its run, the slabs are its own — and so is the configuration
        ctx.run()
        ctx.upload_wide_device_async(dev.data_ptr(), Cn, T, T * R)
        ctx.front(channels=Cn, samples=T)
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        assert _config(ctx, FEED_S, R, wl.IQ_I16, taps) == ESTATE
        ctx.run(channels=Cn, samples=T)
        ctx.upload_wait()
        ctx.frames()
        # both families on one stream: the discriminator's block finds the tuner's last z as its carry, and leaves its last sample
        ctx.reset()
        ctx.upload_wide_device(dev.data_ptr(), Cn, T, T * R, FEED_GAIN)
        nb = np.ascontiguousarray(data[wl.IQ_I16][:1, :64].repeat(Cn, axis=0))
        ctx.upload_iq(nb)
        ts = [wl.Tuner(taps, R, int(FEED_FCW[c]), FEED_GAIN) for c in range(Cn)]
        for c in range(Cn):
            ts[c].block(xi[FEED_SRC[c]])
        e = np.stack([iq.discriminate(nb[c], 1.0, ts[c].carry)[0] for c in range(Cn)])
        _assert_words(ctx.download_f32(), e, "a narrowband block behind a wideband one")
    finally:
        ctx.close()


# ---- 5b: the limits m17hip_wide_config accepts, launched ----------------------------------------------------------------------------------------------
# (16, 1024): the largest LDS the kernel is ever asked for (42 880 B); (1, 1024): one plane, the longest chain per plane; (16, 1023): a tap tail of 7
# behind 127 groups of 8; (3, 1024): the last polyphase row holds one tap
LIM_SHAPES = ((16, 1024), (1, 1024), (16, 1023), (3, 1024))
LIM_C, LIM_T = 3, 511   # two tiles and one output
LIM_SRC = np.array([0, 1, 0], dtype=np.uint32)
LIM_FCW = np.array([-0x12345679, 1 << 30, INT32_MIN], dtype=np.int64)
LIM_GAIN = 1.25
F64_EXCLUDED_CAP = 0.02


def _lim_sources(R, fmt, n=LIM_T):
    """Two sources: the carriers the channels on each listen to (tests/test_wide_input.py's signal), so that the float64 bound on y speaks about nearly
    every output."""
    x = np.stack([wl.carriers(R, [LIM_FCW[c] for c in range(LIM_C) if LIM_SRC[c] == s], n, fmt, seed=6095 + s) for s in range(2)])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("R,L", LIM_SHAPES)
def test_tuner_at_the_limits_of_its_configuration(R, L):
    """Shapes the one-hop test stops short of, all three formats, host and device sources: the host form's words; the int16 floats are also within the
    derived bound of the float64 statement (tests/test_wide_input.py), which the reference is asked about first."""
    taps = wl.hamming_taps(L)
    ctx = m17hip.Context(LIM_C, LIM_T)
    try:
        for name, f in FMTS.items():
            x = _lim_sources(R, f)
            exp = wl.tune_channels(x, LIM_SRC, LIM_FCW, taps, R, LIM_GAIN)
            if f == wl.IQ_I16:
                for c in range(LIM_C):
                    worst, excluded = wl.f64_check_y(exp[c], x[LIM_SRC[c]], taps, R, int(LIM_FCW[c]), LIM_GAIN)
                    assert excluded <= F64_EXCLUDED_CAP, (R, L, c, excluded)
            ctx.wide_config(2, R, f, taps)
            ctx.wide_channels(LIM_SRC, LIM_FCW)
            for way in (x, _dev(x)):
                ctx.reset()
                ctx.upload_wide(way, gain=LIM_GAIN)
                got = ctx.download_f32()
                _assert_words(got, exp, (R, L, name))
                if f == wl.IQ_I16:
                    for c in range(LIM_C):
                        worst, _ = wl.f64_check_y(got[c], x[LIM_SRC[c]], taps, R, int(LIM_FCW[c]), LIM_GAIN)
                        print(f"tuner on the device vs float64, R = {R}, L = {L}, channel {c}: y error {worst:.3f} of its bound")
                        assert worst <= 1.0, (R, L, c, worst)
    finally:
        ctx.close()


def test_blocks_far_shorter_than_the_history():
    """(16, 1024): a feed of 1, 2 and 508 outputs — 16, 32 and 8128 samples against a history of 1023 — in place and staged by turns; every block finds what
    the shorter ones before it left of the history, and the concatenation is the one-block result."""
    R, L = 16, 1024
    taps = wl.hamming_taps(L)
    x = _lim_sources(R, wl.IQ_I16)
    whole = wl.tune_channels(x, LIM_SRC, LIM_FCW, taps, R, LIM_GAIN)
    ref = wl.Feeds(x, taps, LIM_SRC, LIM_FCW, R, LIM_GAIN)
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], LIM_T * R
    ctx = m17hip.Context(LIM_C, 508)
    try:
        ctx.wide_config(2, R, wl.IQ_I16, taps)
        ctx.wide_channels(LIM_SRC, LIM_FCW)
        a = 0
        for k, n in enumerate((1, 2, 508)):
            e = ref.block(a, a + n)
            assert np.array_equal(_u32(e), _u32(whole[:, a:a + n]))
            if k == 1:
                ctx.upload_wide_device_async(dev.data_ptr() + a * R * sb, LIM_C, n, W, LIM_GAIN)
                ctx.run(channels=LIM_C, samples=n)
            elif k == 0:
                ctx.upload_wide_device(dev.data_ptr() + a * R * sb, LIM_C, n, W, LIM_GAIN)
            else:
                ctx.upload_wide(x[:, a * R: (a + n) * R], gain=LIM_GAIN)
            _assert_words(ctx.download_f32(), e, ("block", k, n))
            a += n
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["f32", "i16"])
def test_the_last_of_256_sources(fmt):
    """256 sources of 64 outputs at R = 2, channels on sources 255, 128 and 0; every other source of the float array is NaN (of the int16 one: noise of
    its own), so that a channel that read a wrong row — or a raw buffer sized by channels, not by sources — shows."""
    R, S, n = 2, 256, 64
    f = FMTS[fmt]
    src = np.array([255, 128, 0], dtype=np.uint32)
    taps = m17hip.wide_default_taps(R)
    rng = np.random.default_rng(6096)
    if f == wl.IQ_F32:
        x = np.full((S, n * R), np.nan + 1j * np.nan, dtype=np.complex64)
    else:
        x = rng.integers(-32768, 32768, size=(S, n * R, 2)).astype(np.int16)
    for c, s in enumerate(src):
        x[s] = wl.carriers(R, [LIM_FCW[c]], n, f, seed=6097 + c)
    exp = wl.tune_channels(x, src, LIM_FCW, taps, R, LIM_GAIN)
    assert np.isfinite(exp).all() and len(set(_u32(exp[c]).tobytes() for c in range(3))) == 3
    ctx = m17hip.Context(LIM_C, n)
    try:
        ctx.wide_config(S, R, f, taps)
        ctx.wide_channels(src, LIM_FCW)
        for way in (x, _dev(x)):
            ctx.reset()
            ctx.upload_wide(way, gain=LIM_GAIN)
            _assert_words(ctx.download_f32(), exp, (fmt, "host" if way is x else "device"))
    finally:
        ctx.close()


# ---- 6: the example ------------------------------------------------------------------------------------------------------------------------------
def test_example_tunes_on_the_device(chain_case):
    """examples/m17-demod-gpu --wide-i16 --decim 5 --offset-hz 12500: M17Demodulator<float>::wide buffers the wideband and uploads it block by block
    (m17hip_upload_wide, the feed carried on the device); its frame callbacks are the float oracle's on the host form's floats, in order."""
    x, src, fcw, pol, y, exp = chain_case
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe, "--wide-i16", "--decim", "5", "--offset-hz", "12500"], input=np.ascontiguousarray(x[0]).tobytes(), capture_output=True, check=True,
                         timeout=120).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    recs, _ = fl.demod(y[1])
    e = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == e and len(e) >= 6
