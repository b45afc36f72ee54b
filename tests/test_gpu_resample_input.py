"""GPU tests of wideband IQ input at rational sample rates (ABI 615, include/m17hip.h: m17hip_wide_resample): resample_kernel mixes, filters and decimates,
resamples by up / down and discriminates into the float input slab.  Every comparison is exact: the floats (m17hip_download_f32) as uint32 words against the
HOST form of the same arithmetic (tests/cxx/resample_oracle.cpp: detail/core.h's ddc_resample under the host compiler) — NaN-ness where that is a NaN — and
records, m17_diag and the diagnostic log byte for byte against the float oracle stepped on the host form's floats.  What the host form itself is worth is
asserted without a GPU in tests/test_resample_input.py.  The helpers of tests/test_gpu_wide_input.py and tests/test_gpu_wide2_input.py are imported as they
stand."""
import ctypes as C
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import resample_lib as rl
import test_gpu_wide2_input as g2
import test_gpu_wide_input as g1
import test_resample_input as cpu
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS = g1.FMTS
SB = g1.SB
GAINS = g1.GAINS
INT32_MIN = -(1 << 31)
NAMES = g1.NAMES
_u32, _assert_words, _dev, _raw = g1._u32, g1._assert_words, g1._dev, g1._raw


def _resample(ctx, S, R1, taps1, U, D, taps2, fmt):
    t1 = None if taps1 is None else np.ascontiguousarray(taps1, dtype=np.float32)
    t2 = None if taps2 is None else np.ascontiguousarray(taps2, dtype=np.float32)
    return ctx.lib.m17hip_wide_resample(ctx.h, C.c_uint32(S), C.c_uint32(R1), None if t1 is None else ol._p(t1), C.c_uint32(0 if t1 is None else t1.size),
                                        C.c_uint32(U), C.c_uint32(D), None if t2 is None else ol._p(t2), C.c_uint32(0 if t2 is None else t2.size),
                                        C.c_int(fmt))


def _taps(rng, L):
    return (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)


# ---- 7: one hop ----------------------------------------------------------------------------------------------------------------------------------
# (decim1, up, down, ntaps1, ntaps2): trivial; small; up = down — 5 / 5 has a common factor, which m17hip_wide_resample refuses (only 1 / 1 is up = down
# in lowest terms): the case asserts that refusal, and 5 / 6 beside it is the nearest ratio the configuration accepts —; 2.048 MSPS; 2.5 MSPS; the longest
# history under the smallest tile; the limits
HOP_CASES = [(1, 1, 1, 1, 1), (2, 2, 3, 5, 7), (3, 5, 5, 7, 11), (3, 5, 6, 7, 11), (8, 3, 16, 65, 513), (5, 12, 125, 41, 4001), (16, 1, 125, 256, 4096),
             (16, 32, 125, 256, 4096)]
HOP_ALL_FORMATS = HOP_CASES[:5]
HOP_FEW_CHANNELS = HOP_CASES[6:]   # (3 channels: the host form stays within seconds)
HOP_S, HOP_C = g2.HOP_S, g2.HOP_C
HOP_CN = (1, 3, 65)
BAD_SRC = g2.BAD_SRC
HOP_SRC = g2.HOP_SRC


def _hop_params():
    out = []
    for case in HOP_CASES:
        for name in (list(FMTS) if case in HOP_ALL_FORMATS else ["i16"]):
            out.append(pytest.param(case, name, id="{}_{}over{}_{}_{}-{}".format(*case, name)))
    return out


def _hop_ts(case):
    """U, 2 U and the tile's edges: T - U, T, T + U, 2 T + U for the restated tile of T outputs (only those above 0, each once)."""
    R1, U, D, L1, L2 = case
    T = rl.tile_outputs(L1, R1, L2, U, D)
    return sorted({t for t in (U, 2 * U, T - U, T, T + U, 2 * T + U) if t > 0}), T


@pytest.mark.parametrize("case,fmt", _hop_params())
def test_resampler_one_hop(case, fmt):
    """Host and device sources, pitch larger than the row with rows that are not 16-byte aligned, both gains, every tile edge, 3 sources with 1, 3 and 65
    channels (several on one source, one source unheard; frequency words 0, +-2^30, INT32_MIN, +-1 and random ones): the host form's words.  The float rows
    hold values up to 1e9, denormals and zeroes; one source infinities and NaNs, which stay in the channels that listen to it."""
    R1, U, D, L1, L2 = case
    f = FMTS[fmt]
    ts, tile = _hop_ts(case)
    Tmax = max(ts)
    chans = 3 if case in HOP_FEW_CHANNELS else HOP_C
    rng = np.random.default_rng(6150 + 7 * f + R1 * D + U + L2)
    W = rl.row_len(Tmax, R1, U, D)
    P = W + 3   # odd: row 1 of int16 / uint8 and no float row but 0 and 2 begins 16-byte aligned (a sample is aligned to its own size, no more)
    host = g2._hop_data(f, P, rng)
    dev = _dev(host)
    fcw = rng.integers(INT32_MIN, 1 << 31, HOP_C).astype(np.int64)
    fcw[:6] = (0, 1 << 30, -(1 << 30), INT32_MIN, 1, -1)
    taps1, taps2 = _taps(rng, L1), _taps(rng, L2)
    exp = {g: np.stack([rl.resample(host[HOP_SRC[c]][:W], taps1, R1, U, D, taps2, int(fcw[c]), g) for c in range(chans)]) for g in GAINS}
    if f == wl.IQ_F32:   # (sample 3 of the bad source is infinite: the first outputs hold it whatever the taps)
        e = exp[1.0]
        assert np.isnan(e[BAD_SRC::2]).any() and np.isfinite(e[0::2]).all()
    ctx = m17hip.Context(HOP_C, Tmax)
    try:
        if gcd(U, D) != 1:   # (the host form has words for it; the configuration is refused, and nothing is configured)
            assert _resample(ctx, HOP_S, R1, taps1, U, D, taps2, f) == EINVAL
            assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), 1, U, P) == ESTATE and ctx.iq_bytes() == 0
            return
        assert _resample(ctx, HOP_S, R1, taps1, U, D, taps2, f) == 0
        ctx.wide_channels(HOP_SRC, fcw)
        for ti, T in enumerate(ts):
            Cn = min(65 if T == Tmax else HOP_CN[ti % 3], chans)
            for k, way in enumerate(("host", "device")):
                gain = GAINS[(ti + k) & 1]
                ctx.reset()   # (a fresh feed: histories, count and carries are zero; every T is a prefix of the one expectation)
                name, ptr = ("m17hip_upload_wide", host.ctypes.data) if way == "host" else ("m17hip_upload_wide_device", dev.data_ptr())
                assert _raw(ctx, name, ptr, Cn, T, P, gain) == 0
                ctx.C, ctx.T = Cn, T
                assert ctx.input_format()[0] == m17hip.FORMAT_F32
                _assert_words(ctx.download_f32(), exp[gain][:Cn, :T], (case, fmt, tile, Cn, T, gain, way))
    finally:
        ctx.close()


# ---- 8: up = 1 is the two-stage tuner on the device too --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(10, 5, 81, 161), (16, 16, 256, 700)], ids=["10x5", "16x16"])
def test_up_1_gives_the_words_of_wide_config2_on_the_same_rows_and_table(case):
    R1, R2, L1, L2 = case
    R = R1 * R2
    rng = np.random.default_rng(6160 + R)
    ts = (1, 255, 256, 511)
    P = max(ts) * R + 3
    host = g2._hop_data(wl.IQ_I16, P, rng)
    dev = _dev(host)
    Cn = 5
    fcw = rng.integers(INT32_MIN, 1 << 31, Cn).astype(np.int64)
    fcw[1] = INT32_MIN
    src = HOP_SRC[:Cn]
    taps1, taps2 = _taps(rng, L1), _taps(rng, L2)
    ctx = m17hip.Context(Cn, max(ts))
    try:
        words = {}
        for kind in ("config2", "resample"):
            if kind == "config2":
                assert g2._config2(ctx, HOP_S, R1, taps1, R2, taps2, wl.IQ_I16) == 0
            else:
                assert _resample(ctx, HOP_S, R1, taps1, 1, R2, taps2, wl.IQ_I16) == 0
            ctx.wide_channels(src, fcw)
            for T in ts:
                ctx.reset()
                assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), Cn, T, P, GAINS[1]) == 0
                ctx.C, ctx.T = Cn, T
                words[kind, T] = ctx.download_f32().copy()
        for T in ts:
            _assert_words(words["resample", T], words["config2", T], (case, T))
        assert np.isfinite(words["config2", max(ts)]).all() and np.unique(_u32(words["config2", max(ts)])).size > 1000
    finally:
        ctx.close()


# ---- 9: the feed ---------------------------------------------------------------------------------------------------------------------------------
FEED_CASES = [(8, 3, 16, 65, 513), (5, 12, 125, 41, 4001)]
FEED_S, FEED_C = 2, 5
FEED_GROUPS = (1, 2, 85, 1, 100, 3, 67)   # groups of `up` outputs per block
FEED_SRC = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
FEED_HZ = (12500.0, -75000.0, 0.0, 101000.0, -3000.0)
FEED_GAIN = 1.25


def _feed_case(case, seed=6155, groups=sum(FEED_GROUPS)):
    R1, U, D, L1, L2 = case
    rng = np.random.default_rng(seed + R1 * D)
    x = rng.integers(-20000, 20001, size=(FEED_S, groups * R1 * D, 2)).astype(np.int16)
    taps1, taps2 = _taps(rng, L1), _taps(rng, L2)
    fcw = np.array([m17hip.wide_fcw(h, R1 * D / U) for h in FEED_HZ], dtype=np.int64)
    x.setflags(write=False)
    return x, taps1, taps2, fcw


@pytest.mark.parametrize("case", FEED_CASES, ids=["2048k", "2500k"])
def test_blocks_continue_one_another_across_the_main_and_the_copy_stream(case):
    """Blocks of up x (1, 2, 85, 1, 100, 3, 67) outputs — in place from device memory, staged from device and from pinned memory, and through the host form
    by turns: each finds the sources' histories and the channels' carries the block before it left, whichever stream that ran on.  Checked block by block
    against the host form fed the same blocks, and the concatenation is the one-block result."""
    import torch
    R1, U, D, L1, L2 = case
    x, taps1, taps2, fcw = _feed_case(case)
    whole = rl.resample_channels(x, FEED_SRC, fcw, taps1, R1, U, D, taps2, FEED_GAIN)
    ref = rl.Feeds(x, taps1, R1, U, D, taps2, FEED_SRC, fcw, FEED_GAIN)
    dev = _dev(x)
    pin = torch.from_numpy(np.array(x)).pin_memory()
    sb, W = SB[wl.IQ_I16], x.shape[1]
    cuts = (U * np.cumsum((0,) + FEED_GROUPS)).tolist()
    assert rl.hist_len(L1, R1, L2, U) > 2 * R1 * D   # (the blocks of one and two groups are shorter than the history)
    ctx = m17hip.Context(FEED_C, U * max(FEED_GROUPS))
    try:
        ctx.wide_resample(FEED_S, R1, U, D, wl.IQ_I16, taps1, taps2)
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()
        how = ["in_place", "staged_device", "host", "staged_pinned", "staged_device", "in_place", "staged_pinned"]
        for (a, b), h in zip(zip(cuts[:-1], cuts[1:]), how):
            lo, hi = rl.row_len(a, R1, U, D), rl.row_len(b, R1, U, D)
            off = lo * sb
            if h == "in_place":
                ctx.upload_wide_device(dev.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
            elif h == "host":
                ctx.upload_wide(x[:, lo:hi], gain=FEED_GAIN)
                assert (ctx.C, ctx.T) == (FEED_C, b - a)
            else:
                if h == "staged_device":
                    ctx.upload_wide_device_async(dev.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
                else:
                    ctx.upload_wide_async(pin.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
                ctx.run(channels=FEED_C, samples=b - a)
            e = ref.block(a, b)
            assert np.array_equal(_u32(e), _u32(whole[:, a:b]))
            _assert_words(ctx.download_f32(), e, (case, h, a, b))
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 10: tables, resets, replacement ---------------------------------------------------------------------------------------------------------------
def test_table_changes_resets_and_the_configurations_replacing_one_another():
    case = FEED_CASES[0]
    R1, U, D, L1, L2 = case
    T = 192   # (m17hip_demod_reset_channels wants the context's position on the tick grid; 192 is 3 x 64)
    GW = T // U * D * R1   # wideband samples of a block
    x, taps1, taps2, fcw = _feed_case(case, seed=6156, groups=10 * T // U)
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ratio = R1 * D / U
    ctx = m17hip.Context(FEED_C, GW // R1)
    mk = lambda data, src, w: rl.Feeds(data, taps1, R1, U, D, taps2, src, w, FEED_GAIN)
    ref = mk(x, FEED_SRC, fcw)
    try:
        ctx.wide_resample(FEED_S, R1, U, D, wl.IQ_I16, taps1, taps2)
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()
        ctx.timing(True)

        def up(k, staged=False, n=T):
            getattr(ctx, "upload_wide_device_async" if staged else "upload_wide_device")(dev.data_ptr() + k * GW * sb, FEED_C, n, W, FEED_GAIN)

        up(0)
        _assert_words(ctx.download_f32(), ref.block(0, T), "block 0")
        # the other tables and the survey belong to a raster
        assert ctx.lib.m17hip_wide_raster_channels(ctx.h, ol._p(np.zeros(1, dtype=np.uint32)), ol._p(np.zeros(1, dtype=np.int32)), C.c_uint32(1)) == ESTATE
        assert ctx.lib.m17hip_wide_survey(ctx.h, C.c_uint32(4)) == ESTATE
        # a retune between blocks: channel 0 to another offset, channel 1 to the other source; the first output behind it is one sample of mismatch, nothing more
        old = mk(x, FEED_SRC, fcw)
        old.block(0, T)
        ctx.wide_channels([0, 0], [m17hip.wide_fcw(-400000.0, ratio), fcw[1]])
        ref.src[1], ref.fcw[0] = 0, m17hip.wide_fcw(-400000.0, ratio)
        up(1)
        e1, o1 = ref.block(T, 2 * T), old.block(T, 2 * T)
        assert not np.array_equal(_u32(e1[:2]), _u32(o1[:2])) and np.array_equal(_u32(e1[2:]), _u32(o1[2:]))
        fresh = rl.resample_channels(x, ref.src[:2], ref.fcw[:2], taps1, R1, U, D, taps2, FEED_GAIN)[:, T:2 * T]   # (on the new table from the feed's beginning)
        assert np.array_equal(_u32(e1[:2, 1:]), _u32(fresh[:, 1:])) and not np.array_equal(_u32(e1[:2, 0]), _u32(fresh[:, 0]))
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
        # demod_reset: count, histories and carries start over — a fresh host form on the same table
        ctx.reset()
        up(5)
        f5 = mk(x[:, 5 * GW:], ref.src, ref.fcw)
        e5 = f5.block(0, T)
        assert not np.array_equal(_u32(e5), _u32(ref.block(5 * T, 6 * T)))
        _assert_words(ctx.download_f32(), e5, "block 5, after reset")
        # wide_resample again starts the sources over and leaves the carries
        assert _resample(ctx, FEED_S, R1, taps1, U, D, taps2, wl.IQ_I16) == 0
        up(6)
        f6 = mk(x[:, 6 * GW:], ref.src, ref.fcw)
        f6.carry = [c.copy() for c in f5.carry]
        _assert_words(ctx.download_f32(), f6.block(0, T), "block 6, after a second wide_resample")
        assert ctx.timing_get("resample")[1] == 7 and ctx.timing_get("tune2")[1] == 0 and ctx.timing_get("tune")[1] == 0
        assert ctx.timing_get("channelise")[1] == 0 and ctx.timing_get("discriminate")[1] == 0
        # wide_config2 takes over: the two-stage tuner at decim1 x 4 with the first stage's taps and a second stage of its own, wide2_lib's words (the
        # frequency words now mean fcw / 2^32 * 48000 * decim1 * 4 Hz), the carries still the channels' last z
        rng = np.random.default_rng(6157)
        t2 = _taps(rng, 33)
        assert g2._config2(ctx, FEED_S, R1, taps1, 4, t2, wl.IQ_I16) == 0
        n7 = GW // (R1 * 4)   # (the same samples per source)
        up(7, n=n7)
        f7 = w2.Feeds2(x[:, 7 * GW:], taps1, R1, t2, 4, ref.src, ref.fcw, FEED_GAIN)
        f7.carry = [c.copy() for c in f6.carry]
        ctx.C, ctx.T = FEED_C, n7
        _assert_words(ctx.download_f32(), f7.block(0, n7), "block 7, after wide_config2")
        assert ctx.timing_get("resample")[1] == 7 and ctx.timing_get("tune2")[1] == 1
        # ... and hands back: the resampler, from a fresh feed of the sources
        assert _resample(ctx, FEED_S, R1, taps1, U, D, taps2, wl.IQ_I16) == 0
        up(8)
        f8 = mk(x[:, 8 * GW:], ref.src, ref.fcw)
        f8.carry = [c.copy() for c in f7.carry]
        ctx.C, ctx.T = FEED_C, T
        _assert_words(ctx.download_f32(), f8.block(0, T), "block 8, after wide_resample again")
        # wide_raster takes over — its tables are its own: wide_channels is refused, the survey is served — and hands back with a fresh table
        ctx.wide_raster(FEED_S, 4, 48, wl.IQ_I16)
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.zeros(1, dtype=np.uint32)), ol._p(np.zeros(1, dtype=np.int32)), C.c_uint32(1)) == ESTATE
        ctx.wide_raster_channels([0], [0])
        ctx.wide_survey(4)
        assert _resample(ctx, FEED_S, R1, taps1, U, D, taps2, wl.IQ_I16) == 0
        assert ctx.lib.m17hip_wide_survey(ctx.h, C.c_uint32(4)) == ESTATE
        up(9)
        f9 = mk(x[:, 9 * GW:], [0] * FEED_C, [0] * FEED_C)   # (a bin is no frequency word: the table is all (0, 0) again)
        f9.carry = [c.copy() for c in f8.carry]
        _assert_words(ctx.download_f32(), f9.block(0, T), "block 9, after wide_raster and back")
        assert ctx.timing_get("resample")[1] == 9 and ctx.timing_get("tune2")[1] == 1 and ctx.timing_get("channelise")[1] == 0
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 11: refusals and memory -----------------------------------------------------------------------------------------------------------------------
def test_state_rules_refusals_memory_and_timing():
    import torch
    case = FEED_CASES[0]
    R1, U, D, L1, L2 = case
    x, taps1, taps2, fcw = _feed_case(case)
    whole = rl.resample_channels(x, FEED_SRC, fcw, taps1, R1, U, D, taps2, FEED_GAIN)
    Cn, T = FEED_C, 384
    W = rl.row_len(T, R1, U, D)
    xi = np.ascontiguousarray(x[:, :W])
    dev, pin = _dev(xi), torch.from_numpy(xi.copy()).pin_memory()
    ptrs = dict(zip(NAMES, (xi.ctypes.data, pin.data_ptr(), dev.data_ptr(), dev.data_ptr())))
    maxC = Cn + 2
    ctx = m17hip.Context(maxC, T + 3)
    try:
        assert ctx.iq_bytes() == 0
        for name in NAMES:   # before any configuration
            assert _raw(ctx, name, ptrs[name], Cn, T, W) == ESTATE, name
        one, t256, t4096 = np.ones(1, dtype=np.float32), np.ones(256, dtype=np.float32), np.ones(4096, dtype=np.float32)
        bad = np.array([1.0, np.nan], dtype=np.float32)

        def cfg(S, d1, t1, n1, up, down, t2, n2, fm):
            return ctx.lib.m17hip_wide_resample(ctx.h, C.c_uint32(S), C.c_uint32(d1), None if t1 is None else ol._p(t1), C.c_uint32(n1), C.c_uint32(up),
                                                C.c_uint32(down), None if t2 is None else ol._p(t2), C.c_uint32(n2), C.c_int(fm))

        # every limit from outside, up > down, a common factor, the NULL / 0 combinations, a non-finite tap in either stage
        for args in ((0, 8, one, 1, 3, 16, one, 1, 1), (257, 8, one, 1, 3, 16, one, 1, 1), (1, 0, one, 1, 3, 16, one, 1, 1), (1, 17, one, 1, 3, 16, one, 1, 1),
                     (1, 8, one, 1, 0, 16, one, 1, 1), (1, 8, one, 1, 33, 125, one, 1, 1), (1, 8, one, 1, 3, 0, one, 1, 1), (1, 8, one, 1, 3, 126, one, 1, 1),
                     (1, 8, one, 1, 17, 16, one, 1, 1), (1, 8, one, 1, 6, 16, one, 1, 1), (1, 8, one, 1, 16, 16, one, 1, 1), (1, 8, one, 1, 25, 125, one, 1, 1),
                     (1, 8, one, 1, 3, 16, one, 1, 0), (1, 8, one, 1, 3, 16, one, 1, 4),
                     (1, 8, one, 0, 3, 16, one, 1, 1), (1, 8, None, 1, 3, 16, one, 1, 1), (1, 8, one, 1, 3, 16, one, 0, 1), (1, 8, one, 1, 3, 16, None, 1, 1),
                     (1, 8, np.ones(257, dtype=np.float32), 257, 3, 16, one, 1, 1), (1, 8, one, 1, 3, 16, np.ones(4097, dtype=np.float32), 4097, 1),
                     (1, 8, bad, 2, 3, 16, one, 1, 1), (1, 8, one, 1, 3, 16, bad, 2, 1), (1, 8, one, 1, 3, 16, np.array([np.inf], dtype=np.float32), 1, 1)):
            assert cfg(*args) == EINVAL, args[:2] + args[3:6] + args[7:]
        assert ctx.iq_bytes() == 0
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, W) == ESTATE, name
        # the limits themselves, from inside
        assert cfg(256, 16, t256, 256, 32, 125, t4096, 4096, 3) == 0
        assert cfg(1, 1, one, 1, 1, 1, one, 1, 1) == 0
        assert cfg(1, 16, None, 0, 1, 125, None, 0, 2) == 0 and cfg(1, 8, one, 1, 3, 16, None, 0, 2) == 0 and cfg(1, 8, None, 0, 3, 16, one, 1, 2) == 0
        # memory: the carry; both stages' taps, two histories of H = (ceil(L2 / up) - 1) decim1 + L1 - 1 and the z of a launch
        ctx.wide_resample(FEED_S, R1, U, D, wl.IQ_I16, taps1, taps2)
        H = rl.hist_len(L1, R1, L2, U)
        assert H == (171 - 1) * 8 + 64
        held = ctx.iq_bytes()
        assert held == maxC * 8 + (L1 + L2) * 4 + 2 * FEED_S * H * 8 + maxC * 8
        g1._config(ctx, FEED_S, R1, wl.IQ_I16, taps1)
        assert ctx.iq_bytes() == maxC * 8 + L1 * 4 + 2 * FEED_S * (L1 - 1) * 8 + maxC * 8, "wide_config gives the second stage's memory back"
        ctx.wide_resample(FEED_S, R1, U, D, wl.IQ_I16, taps1, taps2)
        assert ctx.iq_bytes() == held
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()
        # timing index 13 counts this tuner's launches, the other tuners' indices do not
        ctx.timing(True)
        ctx.upload_wide_device(dev.data_ptr(), Cn, T, W, FEED_GAIN)
        assert ctx.iq_bytes() == held + 2 * maxC * 4, "the device forms add one copy of the channel table"
        _assert_words(ctx.download_f32(), whole[:, :T], "device")
        ctx.reset()
        ctx.upload_wide(xi, gain=FEED_GAIN, channels=Cn)
        assert ctx.iq_bytes() == held + 2 * maxC * 4 + FEED_S * W * 4, "and the host forms the raw block"
        _assert_words(ctx.download_f32(), whole[:, :T], "host")
        ms, launches = ctx.timing_get("resample")
        assert launches == 2 and ms > 0, "one launch per block"
        assert ctx.timing_get("tune")[1] == 0 and ctx.timing_get("tune2")[1] == 0 and ctx.timing_get("discriminate")[1] == 0
        ctx.timing(False)
        # the argument refusals, every way in: outputs that are no multiple of `up`, and a pitch one short of samples / up * down * decim1
        for name in NAMES:
            p = ptrs[name]
            assert _raw(ctx, name, None, Cn, T, W) == EINVAL, name
            assert _raw(ctx, name, p, 0, T, W) == EINVAL, name
            assert _raw(ctx, name, p, Cn, 0, W) == EINVAL, name
            assert _raw(ctx, name, p, maxC + 1, T, W) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T + 1, 2 * W) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T + 2, 2 * W) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T - 1, W) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T + 6, 2 * W) == EINVAL, name   # (above the context's samples)
            assert _raw(ctx, name, p, Cn, T, W - 1) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T, W, float("nan")) == EINVAL, name
        # between m17hip_demod_front and its run the slabs are the run's — and so is the configuration
        ctx.run()
        ctx.upload_wide_device_async(dev.data_ptr(), Cn, T, W)
        ctx.front(channels=Cn, samples=T)
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, W) == ESTATE, name
        assert _resample(ctx, FEED_S, R1, taps1, U, D, taps2, wl.IQ_I16) == ESTATE
        ctx.run(channels=Cn, samples=T)
        ctx.upload_wait()
        ctx.frames()
    finally:
        ctx.close()


def test_a_row_of_2_to_the_32_samples_is_refused():
    """3 x 2^22 outputs at 16 x 64 / 3 are 2^32 complex samples per row: the kernels count a row's samples in 32 bits.  Refused on the arguments alone, before
    the pointer is looked at, whatever the pitch; at 15 x 64 / 3 the same block is 2^32 - 2^28 samples and the refusal is only the pitch's."""
    T = 3 << 22
    ctx = m17hip.Context(1, T)
    one = np.ones(1, dtype=np.float32)
    dummy = np.zeros(16, dtype=np.int16)
    try:
        assert _resample(ctx, 1, 16, one, 3, 64, one, wl.IQ_I16) == 0
        for name in NAMES:
            assert _raw(ctx, name, dummy.ctypes.data, 1, T, 1 << 32) == EINVAL, name
            assert _raw(ctx, name, dummy.ctypes.data, 1, T, 1 << 33) == EINVAL, name
        assert _resample(ctx, 1, 15, one, 3, 64, one, wl.IQ_I16) == 0
        assert _raw(ctx, NAMES[0], dummy.ctypes.data, 1, T, (1 << 32) - (1 << 28) - 1) == EINVAL
    finally:
        ctx.close()


# ---- 12: the full chain at 2.048 MSPS --------------------------------------------------------------------------------------------------------------
CH_R1, CH_U, CH_D = cpu.CH_R1, cpu.CH_U, cpu.CH_D
CH_RATIO = CH_R1 * CH_D / CH_U
CH_GROUP = CH_R1 * CH_D   # wideband samples under CH_U outputs
CH_OFFSETS = cpu.OFFSETS
CH_C = 6   # channels 0..2: the three transmissions on source 0; 3..5: the same on source 1 — the spectrum flipped — at the mirrored offsets, inverted


@pytest.fixture(scope="module")
def chain_case():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in cpu.KINDS]
    x0 = cpu.source_2048k(bb)
    x = np.stack([x0, x0 * np.array([1, -1], dtype=np.int16)])
    src = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint32)
    fcw = np.array([m17hip.wide_fcw(f, CH_RATIO) for f in CH_OFFSETS] + [m17hip.wide_fcw(-f, CH_RATIO) for f in CH_OFFSETS], dtype=np.int64)
    pol = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8)
    taps1, taps2 = m17hip.wide_resample_default_taps(CH_R1, CH_U, CH_D)
    y = rl.resample_channels(x, src, fcw, taps1, CH_R1, CH_U, CH_D, taps2, 1.0)
    exp = g1.Expect(y, invert=pol)
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
        ctx.wide_resample(2, CH_R1, CH_U, CH_D)   # (int16, the default taps of both stages)
        ctx.wide_channels(src, fcw)
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_wide(x if src_kind == "host" else _dev(x))
        assert ctx.T == T
        _assert_words(ctx.download_f32(), y, src_kind)
        ctx.run()
        rows, logs = exp.run(0, T)
        g1._check(ctx, rows, logs, src_kind, cap, diags=exp.diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
def test_full_chain_pipelined_in_ragged_segments(chain_case, order):
    """A live feed: m17hip_upload_wide_device_async of segment k + 1, m17hip_demod_front, run — the resampler of the next segment on the copy stream beside
    the state-machine half of the current run; segments of ragged multiples of 192 (a multiple of `up`), mixed polarity."""
    x, src, fcw, pol, y, exp = chain_case
    T = y.shape[1]
    b = [0, 192, 192 * 27, 192 * 28, 192 * 75, 192 * 120, T]
    assert T > b[-2] and T % CH_U == 0
    lens = [b1 - b0 for b0, b1 in zip(b[:-1], b[1:])]
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(CH_C, max(lens))
    try:
        ctx.wide_resample(2, CH_R1, CH_U, CH_D)
        ctx.wide_channels(src, fcw)
        ctx.set_channel_polarity(pol)
        ctx.reset()

        def stage(k):
            ctx.upload_wide_device_async(dev.data_ptr() + b[k] // CH_U * CH_GROUP * sb, CH_C, lens[k], W)

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
            g1._check(ctx, rows, None, f"pipelined {order}, segment {k}", 0, diags=None if more else exp.diags, got=got)
            if more and order != "run_then_fetch":
                ctx.run(channels=CH_C, samples=lens[k + 1])
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


# ---- 13: the example -------------------------------------------------------------------------------------------------------------------------------
def test_example_tunes_a_2048k_source_on_the_device(chain_case):
    """examples/m17-demod-gpu --wide-i16 --rate 2048000 --offset-hz 12500: M17Demodulator<float>::wide_rate asks m17hip_wide_resample_ratio for the shape
    (16 x 3 / 8), buffers whole groups of outputs and uploads them block by block (m17hip_wide_resample, the feed carried on the device); its frame callbacks
    are the float oracle's on the host form's floats at that shape, in order."""
    x, src, fcw, pol, y, exp = chain_case
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    assert m17hip.wide_resample_ratio(2048000) == (16, 3, 8)
    out = subprocess.run([exe, "--wide-i16", "--rate", "2048000", "--offset-hz", "12500"], input=np.ascontiguousarray(x[0]).tobytes(),
                         capture_output=True, check=True, timeout=120).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    taps1, taps2 = m17hip.wide_resample_default_taps(16, 3, 8)
    recs, _ = fl.demod(rl.resample(x[0], taps1, 16, 3, 8, taps2, m17hip.wide_fcw(12500.0, 128 / 3)))
    e = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == e and len(e) >= 6
