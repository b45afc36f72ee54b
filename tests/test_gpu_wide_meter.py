"""GPU tests of the channel meter (ABI 618, include/m17hip.h: m17hip_wide_meter): the metered instantiations of tune_kernel, tune2_kernel, resample_kernel
and chan_kernel store chan_power of every z they discriminate, and wide_meter_kernel sums it, the stored y and y * y per channel and piece of a window.
Every comparison is exact: the planes (m17hip_wide_meter_fetch) as uint32 words against the HOST form of the same arithmetic (tests/meter_lib.py:
detail/core.h under the host compiler, over the z and y of the four configurations' host forms) — NaN-ness where that is a NaN.  What the host form
itself is worth is asserted without a GPU in tests/test_wide_meter.py.  The helpers of tests/test_gpu_wide_input.py and tests/test_gpu_raster_input.py
are imported as they stand."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import meter_lib as ml
import oracle_lib as ol
import raster_lib as ra
import resample_lib as rl
import test_gpu_raster_input as gr
import test_gpu_wide_input as g1
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS, SB = g1.FMTS, g1.SB
_data, _dev, _raw = gr._data, gr._dev, gr._raw
_u32, _assert_words = g1._u32, g1._assert_words
NAMES = ("m17hip_upload_wide", "m17hip_upload_wide_async", "m17hip_upload_wide_device", "m17hip_upload_wide_device_async")
GAIN = 5.0 / 3.0
LICH = 1


def _shape(ctx, back=0):
    c, k, t = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
    fw, fo = C.c_uint64(0xFFFFFFFFFFFFFFFF), C.c_uint64(0xFFFFFFFFFFFFFFFF)
    code = ctx.lib.m17hip_wide_meter_shape(ctx.h, C.c_uint32(back), C.byref(c), C.byref(k), C.byref(fw), C.byref(fo), C.byref(t))
    return code, (c.value, k.value, fw.value, fo.value, t.value)


def _fetch_code(ctx, back=0, n=64):
    buf = np.full(n, 7.0, dtype=np.float32)
    code = ctx.lib.m17hip_wide_meter_fetch(ctx.h, C.c_uint32(back), ol._p(buf), C.c_uint64(n))
    assert code == 0 or (buf == 7.0).all()   # (a refusal writes nothing)
    return code


def _expect(ctx, P, Y, a, b, N0, window, what, back=0):
    """The plane `back` names is the host form's of the feed's outputs a .. b - 1 that begin at output N0, and its shape says so."""
    exp = ml.planes(P, Y, a, b, N0, window)
    code, shape = _shape(ctx, back)
    assert code == 0, (what, code)
    assert shape == (P.shape[0], exp.shape[2], N0 // window, N0, b - a), (what, shape)
    got, fw, fo, t = ctx.wide_meter_fetch(back)
    assert got.shape == exp.shape and got.dtype == np.float32 and (fw, fo, t) == shape[2:], what
    _assert_words(got, exp, what)
    assert (m17hip.wide_meter_counts(fo, t, window) == [m for _, m in ml.pieces_stated(N0, b - a, window)]).all()


# ---- the four configurations: what configures them, and the host form's p and y of a whole feed ---------------------------------------------------------
class Setup:
    """kind, sources, channels; `u` outputs and `g` source samples per group; configure(ctx, fmt) and feed(data) -> (P[C][n], Y[C][n])."""


def _tuner1():
    s = Setup()
    s.kind, s.S, s.u, s.g = "config", 2, 1, 5
    s.src = [0, 0, 0, 1, 1, 1]
    # two share a source and a word; one sits on each source's edge (-Fs / 2 and the last word below +Fs / 2)
    s.fcw = [m17hip.wide_fcw(30000.0, 5), m17hip.wide_fcw(30000.0, 5), -(1 << 31), (1 << 31) - 1, m17hip.wide_fcw(-47000.0, 5), 12345]
    taps = m17hip.wide_default_taps(5)

    def configure(ctx, fmt):
        ctx.wide_config(s.S, 5, fmt)
        ctx.wide_channels(s.src, s.fcw)

    def feed(data):
        got = [wl.Tuner(taps, 5, w, GAIN).block(data[c], want_z=True) for c, w in zip(s.src, s.fcw)]
        return np.stack([ml.power(z) for _, z in got]), np.stack([y for y, _ in got])
    s.configure, s.feed = configure, feed
    return s


def _tuner2():
    s = Setup()
    s.kind, s.S, s.u, s.g = "config2", 2, 1, 6
    s.src, s.fcw = [1, 0, 1], [m17hip.wide_fcw(40000.0, 6), m17hip.wide_fcw(-100000.0, 6), -(1 << 31)]
    t1, t2 = m17hip.wide_default_taps2(2, 3)

    def configure(ctx, fmt):
        ctx.wide_config2(s.S, 2, 3, fmt)
        ctx.wide_channels(s.src, s.fcw)

    def feed(data):
        got = [w2.Tuner2(t1, 2, t2, 3, w, GAIN).block(data[c], want_z=True) for c, w in zip(s.src, s.fcw)]
        return np.stack([ml.power(z) for _, z in got]), np.stack([y for y, _ in got])
    s.configure, s.feed = configure, feed
    return s


def _resampler():
    s = Setup()
    s.kind, s.S, s.u, s.g = "resample", 2, 3, 8 * 16   # 2.048 MSPS: decim1 16, up 3, down 8
    s.src, s.fcw = [0, 1, 1], [m17hip.wide_fcw(-762500.0, 128 / 3), m17hip.wide_fcw(12500.0, 128 / 3), (1 << 31) - 1]
    t1, t2 = m17hip.wide_resample_default_taps(16, 3, 8)

    def configure(ctx, fmt):
        ctx.wide_resample(s.S, 16, 3, 8, fmt)
        ctx.wide_channels(s.src, s.fcw)

    def feed(data):
        got = [rl.Resampler(t1, 16, 3, 8, t2, w, GAIN).block(data[c], want_z=True) for c, w in zip(s.src, s.fcw)]
        return np.stack([ml.power(z) for _, z in got]), np.stack([y for y, _ in got])
    s.configure, s.feed = configure, feed
    return s


RASTER_L = 4001   # taps that leave the channeliser a tile of 24 outputs (under its 31)


def _raster():
    s = Setup()
    s.kind, s.S, s.u, s.g = "raster", 2, 1, 64
    # four channels in the table — two on one bin of source 0 —, three in the launch: bin 3 of source 1 is in the table and nobody listens
    s.src, s.bins, s.table_src, s.table_bins = [0, 0, 1], [5, 5, -7], [0, 0, 1, 1], [5, 5, -7, 3]
    taps = wl.hamming_taps(RASTER_L)
    assert ra.tile_and_lds(RASTER_L, 64, 48)[0] == 24

    def configure(ctx, fmt):
        ctx.wide_raster(s.S, 64, 48, fmt, taps)
        ctx.wide_raster_channels(s.table_src, s.table_bins)

    def feed(data):
        P, Y = [], []
        for c, (src, b) in enumerate(zip(s.src, s.bins)):
            y, z = ra.Raster(taps, 64, 48, [b], GAIN).block(data[src], want_z=True)
            P.append(ml.power(z[0]))
            Y.append(y[0])
        return np.stack(P), np.stack(Y)
    s.configure, s.feed = configure, feed
    return s


SETUPS = {"config": _tuner1, "config2": _tuner2, "resample": _resampler, "raster": _raster}
BLOCKS = {"config": (547, 16, 1, 255), "config2": (3 * 255 * 2 + 15, 3), "resample": (3 * 255 * 2 + 15, 3), "raster": (2 * 24 + 5, 7)}


@functools.lru_cache(maxsize=None)
def _case(kind, fmt):
    """(setup, data [S][W] read-only, P, Y) of one feed of BLOCKS[kind], made once and shared."""
    s = SETUPS[kind]()
    n = sum(BLOCKS[kind])
    rng = np.random.default_rng(6180 + len(kind) + fmt)
    data = _data(fmt, s.S, n // s.u * s.g, rng)
    P, Y = s.feed(data)
    assert P.shape == (len(s.src), n) and Y.shape == P.shape
    for a in (data, P, Y):
        a.setflags(write=False)
    return s, data, P, Y


def _feed_blocks(ctx, s, dev, fmt, blocks, windows, P, Y, what, channels=None):
    """Uploads the blocks in place from device memory, the meter at windows[k] for block k; every plane against the host form."""
    Cn = len(s.src) if channels is None else channels
    sb, pitch = SB[fmt], dev.shape[1]
    a = 0
    for k, n in enumerate(blocks):
        if k == 0 or windows[k] != windows[k - 1]:
            ctx.wide_meter(windows[k])
        assert _raw(ctx, NAMES[2], dev.data_ptr() + a // s.u * s.g * sb, Cn, n, pitch, GAIN) == 0, (what, k)
        ctx.C, ctx.T = Cn, n
        _expect(ctx, P[:Cn], Y[:Cn], a, a + n, a, windows[k], (what, k))
        a += n


# ---- 1: the one-stage tuner ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", (16, 48, 1920))
def test_one_stage_tuner_int16(window):
    """2 int16 sources at R = 5 with the default taps, six channels, blocks of 547 (two tiles and 37), 16, 1 and 255 outputs of one feed: the windows are cut
    where the FEED's output count says (547 is no multiple of 16 or 48), pieces of one output included."""
    s, data, P, Y = _case("config", wl.IQ_I16)
    ctx = m17hip.Context(len(s.src), max(BLOCKS["config"]))
    try:
        s.configure(ctx, wl.IQ_I16)
        ctx.reset()
        _feed_blocks(ctx, s, _dev(data), wl.IQ_I16, BLOCKS["config"], [window] * 4, P, Y, ("config", window))
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ("f32", "u8"))
def test_one_stage_tuner_other_formats(fmt):
    """The same feed once each from float32 (components up to 1e9, denormals, zeroes of either sign: powers overflow, and the words still agree) and uint8
    sources, the window changing with the block."""
    f = FMTS[fmt]
    s, data, P, Y = _case("config", f)
    ctx = m17hip.Context(len(s.src), max(BLOCKS["config"]))
    try:
        s.configure(ctx, f)
        ctx.reset()
        _feed_blocks(ctx, s, _dev(data), f, BLOCKS["config"], [48, 16, 16, 1920], P, Y, ("config", fmt))
    finally:
        ctx.close()


# ---- 2: the other three configurations ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("config2", "resample", "raster"))
def test_two_stage_resampling_and_channeliser(kind):
    """The two-stage tuner at 2 x 3 and the resampling tuner at 2.048 MSPS (16, 3 / 8) on blocks of 1545 outputs (more than two tiles) and 3 (one group);
    the channeliser at M = 48, decim 64 and 4001 taps (a tile of 24 outputs) on blocks of two tiles and 5 outputs, then 7: two channels on one bin, a
    table of four channels of which the launch takes three.  Windows 16 and 48 by turns, then 1920 over the whole feed again after a reset."""
    s, data, P, Y = _case(kind, wl.IQ_I16)
    blocks = BLOCKS[kind]
    ctx = m17hip.Context(4, max(blocks))
    try:
        dev = _dev(data)
        s.configure(ctx, wl.IQ_I16)
        ctx.reset()
        _feed_blocks(ctx, s, dev, wl.IQ_I16, blocks, [16, 48], P, Y, (kind, "16/48"), channels=len(s.src))
        ctx.reset()   # (the meter stays on at 48; the feed and its windows start over)
        _feed_blocks(ctx, s, dev, wl.IQ_I16, blocks, [1920, 1920], P, Y, (kind, 1920), channels=len(s.src))
    finally:
        ctx.close()


@pytest.mark.parametrize("window", (16, 2047, 4096, 65536))
def test_long_blocks_many_pieces_and_long_pieces(window):
    """wide_config at decim 1 with five taps, two channels, blocks of 49 000 and 17 000 outputs.  Window 16: 3063 and 1063 pieces a channel, twelve and
    five workgroups of 256 pieces.  2047: two pieces per workgroup.  4096: a piece per workgroup, every lane a group.  65 536: one piece of 3063 groups —
    three passes over the kernel's 1024 slots, the second-level chains carried across them — then a0 = 49 000: pieces of 16 536 outputs (1034 groups: two
    passes, the second of ten groups) and 464."""
    rng = np.random.default_rng(6185)
    blocks = (49000, 17000)
    n = sum(blocks)
    data = _data(wl.IQ_I16, 1, n, rng)
    taps = wl.hamming_taps(5)
    fcw = [1 << 28, -(1 << 30) + 77]
    got = [wl.Tuner(taps, 1, w, GAIN).block(data[0], want_z=True) for w in fcw]
    P, Y = np.stack([ml.power(z) for _, z in got]), np.stack([y for y, _ in got])
    ctx = m17hip.Context(2, max(blocks))
    try:
        dev = _dev(data)
        ctx.wide_config(1, 1, wl.IQ_I16, taps)
        ctx.wide_channels([0, 0], fcw)
        ctx.reset()
        ctx.wide_meter(window)
        a = 0
        for k, T in enumerate(blocks):
            assert _raw(ctx, NAMES[2], dev.data_ptr() + a * 4, 2, T, n, GAIN) == 0
            ctx.C, ctx.T = 2, T
            _expect(ctx, P, Y, a, a + T, a, window, (window, k))
            a += T
    finally:
        ctx.close()


# ---- 3: the meter does not change the demodulator's input ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SETUPS))
def test_the_channels_floats_are_the_same_words_with_the_meter_on_and_off(kind):
    s, data, P, Y = _case(kind, wl.IQ_I16)
    blocks = BLOCKS[kind]
    Cn = len(s.src)
    ctx = m17hip.Context(6, max(blocks))
    got = {}
    try:
        dev = _dev(data)
        for on in (False, True):
            s.configure(ctx, wl.IQ_I16)
            ctx.reset()
            if on:
                ctx.wide_meter(48)
            got[on], a = [], 0
            for n in blocks:
                assert _raw(ctx, NAMES[2], dev.data_ptr() + a // s.u * s.g * 4, Cn, n, dev.shape[1], GAIN) == 0
                ctx.C, ctx.T = Cn, n
                got[on].append(ctx.download_f32().copy())
                assert (_shape(ctx)[0] == 0) == on
                a += n
        a = 0
        for off, on_, n in zip(got[False], got[True], blocks):
            assert np.array_equal(_u32(off), _u32(on_)), kind
            _assert_words(on_, Y[:, a:a + n], (kind, "the host form's y"))
            a += n
    finally:
        ctx.close()


# ---- 4: two blocks in flight --------------------------------------------------------------------------------------------------------------------------------
def test_a_staged_and_an_in_place_block_in_flight_then_a_run():
    """One block staged on the copy stream, the next in place on the main stream, no wait in between, then a run: back = 1 and back = 0 are each their own
    host form — the power scratch is one, and the second block's tuner is ordered behind the first block's meter kernel."""
    s, data, P, Y = _case("config", wl.IQ_I16)
    n0, n1 = 547, 255
    ctx = m17hip.Context(len(s.src), n0)
    try:
        dev = _dev(data)
        s.configure(ctx, wl.IQ_I16)
        ctx.reset()
        ctx.wide_meter(48)
        assert _raw(ctx, NAMES[3], dev.data_ptr(), 6, n0, dev.shape[1], GAIN) == 0
        assert _raw(ctx, NAMES[2], dev.data_ptr() + n0 * 5 * 4, 6, n1, dev.shape[1], GAIN) == 0
        ctx.run(channels=6, samples=n0)   # (the staged block's)
        _expect(ctx, P, Y, 0, n0, 0, 48, "staged", back=1)
        _expect(ctx, P, Y, n0, n0 + n1, n0, 48, "in place", back=0)
    finally:
        ctx.close()


# ---- 5: state -----------------------------------------------------------------------------------------------------------------------------------------------
def test_state():
    s, data, P, Y = _case("config", wl.IQ_I16)
    ctx = m17hip.Context(len(s.src), 547)
    lib = ctx.lib
    try:
        dev = _dev(data)
        ptr, pitch = dev.data_ptr(), dev.shape[1]
        assert lib.m17hip_wide_meter(ctx.h, C.c_uint32(48)) == ESTATE   # (no wideband configuration yet)

        def block(a, n):
            assert _raw(ctx, NAMES[2], ptr + a * 5 * 4, 6, n, pitch, GAIN) == 0
            ctx.C, ctx.T = 6, n

        # every configuration call turns it off
        for conf in (lambda: ctx.wide_config(2, 5), lambda: ctx.wide_config2(2, 2, 3), lambda: ctx.wide_raster(2, 5, 48),
                     lambda: ctx.wide_resample(2, 16, 3, 8), lambda: s.configure(ctx, wl.IQ_I16)):
            ctx.wide_config(2, 5)
            ctx.wide_channels(s.src, s.fcw)
            ctx.wide_meter(48)
            block(0, 16)
            assert _shape(ctx)[0] == 0 and _fetch_code(ctx, 0, 3 * 6 * 1) == 0
            conf()
            assert _shape(ctx)[0] == ESTATE and _fetch_code(ctx) == ESTATE
        for bad in (1, 15, 65537, 0xFFFFFFFF):
            assert lib.m17hip_wide_meter(ctx.h, C.c_uint32(bad)) == EINVAL
        # a feed: N0 follows the blocks, back = 1 is the block before, reset starts it over with the meter on
        ctx.reset()
        ctx.wide_meter(48)
        assert _shape(ctx)[0] == ESTATE
        block(0, 100)
        assert _shape(ctx, 1)[0] == ESTATE and _fetch_code(ctx, 2) == EINVAL and _fetch_code(ctx, 0, 3 * 6 * 3 - 1) == EINVAL
        block(100, 17)
        _expect(ctx, P, Y, 100, 117, 100, 48, "the second block")
        _expect(ctx, P, Y, 0, 100, 0, 48, "back = 1", back=1)
        ctx.reset()
        assert _shape(ctx)[0] == ESTATE   # (the planes were blocks of the feed that ended)
        block(0, 100)
        _expect(ctx, P, Y, 0, 100, 0, 48, "after reset")
        # a window change: the next plane has the new shape, the old planes are gone; the plane grows (1920 -> 16 at the same T) under a block in flight
        ctx.wide_meter(1920)
        assert _shape(ctx)[0] == ESTATE and _shape(ctx, 1)[0] == ESTATE
        block(100, 255)
        ctx.wide_meter(16)
        assert _shape(ctx)[0] == ESTATE
        block(355, 255)
        slab = ctx.download_f32().copy()
        _assert_words(slab, Y[:, 355:610], "the block's floats")
        _expect(ctx, P, Y, 355, 610, 355, 16, "window 16")
        assert _shape(ctx, 1)[0] == ESTATE
        # the plane grows because the block does: the block before keeps its words
        block(610, 16)
        block(626, 193)
        _expect(ctx, P, Y, 626, 819, 626, 16, "a larger block")
        _expect(ctx, P, Y, 610, 626, 610, 16, "the block before it", back=1)
        # off: a block queues nothing of the meter's
        ctx.wide_meter(0)
        assert _shape(ctx)[0] == ESTATE
        # memory and timing
        nbytes = ctx.iq_bytes()
        assert nbytes >= 6 * 255 * 4 + 3 * 6 * 16 * 4
        ctx.reset()
        ctx.wide_meter(48)
        ctx.timing(True)
        ctx.timing_reset()
        block(0, 100)
        block(100, 17)
        ctx.wide_meter_fetch()
        ms, launches = ctx.timing_get("meter")
        assert launches == 2 and ms > 0.0
        assert ctx.timing_get("tune")[1] == 2
        ctx.timing(False)
    finally:
        ctx.close()


def test_reset_channels_leaves_the_feeds_count():
    """m17hip_demod_reset_channels zeroes carries, so the listed channels' first y and nothing else differs from the uncut feed: the meter's N0 goes on."""
    s, data, P, Y = _case("config", wl.IQ_I16)
    ctx = m17hip.Context(len(s.src), 547)
    try:
        dev = _dev(data)
        s.configure(ctx, wl.IQ_I16)
        ctx.reset()
        ctx.wide_meter(48)
        assert _raw(ctx, NAMES[2], dev.data_ptr(), 6, 100, dev.shape[1], GAIN) == 0
        ctx.reset_channels([1])
        assert _raw(ctx, NAMES[2], dev.data_ptr() + 100 * 5 * 4, 6, 17, dev.shape[1], GAIN) == 0
        ctx.C, ctx.T = 6, 17
        y = ctx.download_f32()
        Y2 = Y.copy()
        Y2[1, 100] = y[1, 0]   # (against a zero carry: the one word the reset changes)
        assert _shape(ctx)[1][3] == 100
        _expect(ctx, P, Y2, 100, 117, 100, 48, "N0 goes on")
    finally:
        ctx.close()


# ---- 6: through the whole chain -----------------------------------------------------------------------------------------------------------------------------
CHAIN_A, CHAIN_HZ, CHAIN_OFF = 6000.0, 50000.0, 250.0


def test_a_generated_transmission_decodes_and_its_report_is_the_host_forms():
    """One M17 stream transmission through the generator (m17hip_synth_wide at 5 x 48 kSPS, amplitude 6000) 250 Hz above the channel's word: the frames
    decode, and the report over the frames' windows (1920 outputs) is the host form's report.  Equality is the assertion; tests/test_wide_meter.py
    carries the meaning."""
    bb = ol.generate(ol.gen_params(seed=1, kind=1, lead_in=9600, n_frames=6, tail=4800))
    T = bb.size // 1920 * 1920
    bb = bb[:T]
    sent = ol.demod(bb)[0]
    expect = [bytes(p) for p in sent[(sent["cost"] < 30) & (sent["frame_type"] != LICH)]["payload"]]
    tx = m17hip.Context(1, T)
    try:
        tx.upload(bb[None, :])
        tx.synth_wide_config(1, 5, 1, wl.IQ_I16, None, 60.0, 3, 0)
        tx.synth_wide_channels([0], [m17hip.wide_fcw(CHAIN_HZ, 5)], 0, CHAIN_A)
        x = tx.synth_wide().copy()
    finally:
        tx.close()
    fcw = m17hip.wide_fcw(CHAIN_HZ - CHAIN_OFF, 5)
    taps = m17hip.wide_default_taps(5)
    y, z = wl.Tuner(taps, 5, fcw, 1.0).block(x[0], want_z=True)
    P, Y = ml.power(z)[None, :], y[None, :]
    ctx = m17hip.Context(1, T)
    try:
        ctx.wide_config(1, 5)
        ctx.wide_channels([0], [fcw])
        ctx.reset()
        ctx.wide_meter(1920)
        ctx.upload_wide(x, channels=1)
        ctx.run()
        recs = ctx.frames()
        _expect(ctx, P, Y, 0, T, 0, 1920, "the chain")
        planes, fw, fo, t = ctx.wide_meter_fetch()
    finally:
        ctx.close()
    good = recs[(recs["cost"] < 30) & (recs["frame_type"] != LICH)]
    assert len(expect) == 7 and [bytes(p) for p in good["payload"]] == expect   # (the LSF and six stream frames)
    counts = m17hip.wide_meter_counts(fo, t, 1920)
    got = m17hip.wide_meter_report(planes, counts, 1.0)
    exp = m17hip.wide_meter_report(ml.planes(P, Y, 0, T, 0, 1920), counts, 1.0)
    frames = slice(9600 // 1920, (9600 + 7 * 1920) // 1920)   # (the windows the transmission fills)
    for k in ("level_db", "offset_hz", "deviation_hz"):
        assert np.array_equal(got[k], exp[k]) and np.isfinite(got[k][0, frames]).all(), k
    print("chain report over the frames:", {k: np.round(got[k][0, frames], 2).tolist() for k in got})
