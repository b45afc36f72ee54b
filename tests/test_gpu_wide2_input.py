"""GPU tests of wideband IQ input in two decimation stages (ABI 610, include/m17hip.h: m17hip_wide_config2): tune2_kernel mixes, filters and decimates twice
and discriminates into the float input slab.  Every comparison is exact: the floats (m17hip_download_f32) as uint32 words against the HOST form of the same
arithmetic (tests/cxx/wide2_oracle.cpp: detail/core.h's ddc_fir2 under the host compiler) — NaN-ness where that is a NaN — and records, m17_diag and the
diagnostic log byte for byte against the float oracle stepped on the host form's floats.  What the host form itself is worth is asserted without a GPU in
tests/test_wide2_input.py.  The helpers of tests/test_gpu_wide_input.py are imported as they stand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import test_gpu_wide_input as g1
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS = g1.FMTS
SB = g1.SB
GAINS = g1.GAINS
INT32_MIN = -(1 << 31)
_u32, _assert_words, _dev, _raw = g1._u32, g1._assert_words, g1._dev, g1._raw


def _config2(ctx, S, R1, taps1, R2, taps2, fmt):
    t1 = None if taps1 is None else np.ascontiguousarray(taps1, dtype=np.float32)
    t2 = None if taps2 is None else np.ascontiguousarray(taps2, dtype=np.float32)
    return ctx.lib.m17hip_wide_config2(ctx.h, C.c_uint32(S), C.c_uint32(R1), None if t1 is None else ol._p(t1), C.c_uint32(0 if t1 is None else t1.size),
                                       C.c_uint32(R2), None if t2 is None else ol._p(t2), C.c_uint32(0 if t2 is None else t2.size), C.c_int(fmt))


# ---- 1: one hop ----------------------------------------------------------------------------------------------------------------------------------
# (decim1, decim2, ntaps1, ntaps2): no decimation at all; small odd ones; 2.4 MSPS with the default lengths; one stage that does nothing on either side;
# the configuration's limit — 64 KB of LDS with 40 u per chain of a chunk where the others have 64, and it must launch.
HOP_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (10, 5, 81, 161), (16, 1, 129, 33), (3, 16, 1, 513), (16, 16, 256, 1024)]
HOP_ALL_FORMATS = HOP_CASES[:3]
# a tile is 255 outputs: its edges +- 1, two tiles and one output; 100: the u under 100 outputs end inside a chunk of stage 1 for every case here (as they do
# at most other sizes: a tile's u are a multiple of the chunk only by accident), and the tile's last z an output reads lies inside a lane's second chain
HOP_TS = (1, 2, 100, 254, 255, 256, 511)
HOP_S, HOP_C = 3, 65
HOP_CN = (1, 3, 65)
BAD_SRC = 1   # the float source that holds infinities and NaNs: they stay in the channels that listen to it.  Source 2 is heard by nobody.
HOP_SRC = np.array([c % 2 for c in range(HOP_C)], dtype=np.uint32)


def _hop_params():
    out = []
    for case in HOP_CASES:
        for name in (list(FMTS) if case in HOP_ALL_FORMATS else ["i16"]):
            out.append(pytest.param(case, name, id="{}x{}_{}_{}-{}".format(*case, name)))
    return out


def _hop_data(fmt, P, rng):
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
        x = g1._spice(x, rng)
        v = x[BAD_SRC].view(np.float32)
        for k, val in zip(rng.choice(np.arange(40, 2 * P, 97), 9, replace=False), [np.inf, -np.inf, np.nan] * 3):
            v[k] = val
        v[6] = np.inf
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("case,fmt", _hop_params())
def test_two_stage_tuner_one_hop(case, fmt):
    """Host and device sources, pitch > samples * decim1 * decim2 with rows that are not 16-byte aligned, both gains, every tile edge, 3 sources with 1, 3 and
    65 channels (several on one source, one source unheard; frequency words 0, +-2^30, INT32_MIN and random ones) and one source with 3: the host form's
    words.  The float rows hold values up to 1e9, denormals and zeroes; one source infinities and NaNs, which stay in the channels that listen to it."""
    R1, R2, L1, L2 = case
    R, f = R1 * R2, FMTS[fmt]
    rng = np.random.default_rng(6100 + 7 * f + R + L2)
    Tmax = max(HOP_TS)
    P = Tmax * R + 3   # odd: row 1 of int16 / uint8 and no float row but 0 and 2 begins 16-byte aligned (a sample is aligned to its own size, no more)
    host = _hop_data(f, P, rng)
    dev = _dev(host)
    fcw = rng.integers(INT32_MIN, 1 << 31, HOP_C).astype(np.int64)
    fcw[:6] = (0, 1 << 30, -(1 << 30), INT32_MIN, 1, -1)
    taps1 = (rng.standard_normal(L1) / np.sqrt(L1)).astype(np.float32)
    taps2 = (rng.standard_normal(L2) / np.sqrt(L2)).astype(np.float32)
    ctx = m17hip.Context(HOP_C, Tmax)
    try:
        for S in (HOP_S, 1):
            src = np.zeros(HOP_C, dtype=np.uint32) if S == 1 else HOP_SRC
            chans = 3 if S == 1 else HOP_C
            exp = {g: np.stack([w2.tune2(host[src[c]][: Tmax * R], taps1, R1, taps2, R2, int(fcw[c]), g) for c in range(chans)]) for g in GAINS}
            if f == wl.IQ_F32 and S > 1:   # (sample 3 of the bad source is infinite: the first outputs hold it whatever the taps)
                e = exp[1.0]
                assert np.isnan(e[BAD_SRC::2]).any() and np.isfinite(e[0::2]).all()
            assert _config2(ctx, S, R1, taps1, R2, taps2, f) == 0
            ctx.wide_channels(src, fcw)
            for ti, T in enumerate(HOP_TS if S > 1 else (255, 100)):
                Cn = min(65 if T == Tmax else HOP_CN[ti % 3], chans)
                for k, way in enumerate(("host", "device")):
                    gain = GAINS[(ti + k) & 1]
                    ctx.reset()   # (a fresh feed: histories, count and carries are zero)
                    name, ptr = ("m17hip_upload_wide", host.ctypes.data) if way == "host" else ("m17hip_upload_wide_device", dev.data_ptr())
                    assert _raw(ctx, name, ptr, Cn, T, P, gain) == 0
                    ctx.C, ctx.T = Cn, T
                    assert ctx.input_format()[0] == m17hip.FORMAT_F32
                    _assert_words(ctx.download_f32(), exp[gain][:Cn, :T], (case, fmt, S, Cn, T, gain, way))
    finally:
        ctx.close()


# ---- 1b: one hop where a chunk's chains hold fewer than 64 u -------------------------------------------------------------------------------------
# Q < 64 is wide_chains<0> (the chains' distance is not a constant) and chunks of 4 Q u that are no multiple of the wave: (16, 12, 256, 1024) has Q = 56,
# (16, 16, 256, 700) Q = 45 — an odd chunk of 180 u — and the limit Q = 40.  The limit and Q = 45 also from float32 and uint8 rows: the sixteen-load fill
# group of those sample types beside chunks that end inside a group.  (case, expected Q, formats)
LOWQ_CASES = [((16, 12, 256, 1024), 56, ("i16",)), ((16, 16, 256, 700), 45, ("i16", "f32", "u8")), ((16, 16, 256, 1024), 40, ("f32", "u8"))]
LOWQ_TS = (1, 255, 256, 511)
LOWQ_CN = (1, 3)


def _lowq_params():
    return [pytest.param(case, q, name, id="{}x{}_{}_{}-q{}-{}".format(*case, q, name)) for case, q, names in LOWQ_CASES for name in names]


@pytest.mark.parametrize("case,q,fmt", _lowq_params())
def test_two_stage_tuner_one_hop_with_short_chains(case, q, fmt):
    """The configurations whose LDS leaves fewer than 64 u per chain of a stage-1 chunk, from device rows that are not 16-byte aligned, three sources (the
    float one in the middle holds infinities and NaNs), 1 and 3 channels, a tile's edges and two tiles and one output: the host form's words.  What Q and
    how much LDS each configuration has is asserted from the restated layout (wide2_lib.q_and_lds)."""
    R1, R2, L1, L2 = case
    R, f = R1 * R2, FMTS[fmt]
    got_q, lds = w2.q_and_lds(L1, R1, L2, R2)
    assert got_q == q < 64 and lds <= 65536, (case, got_q, lds)
    rng = np.random.default_rng(6110 + 7 * f + R + L2)
    Tmax = max(LOWQ_TS)
    P = Tmax * R + 3
    host = _hop_data(f, P, rng)
    dev = _dev(host)
    Cmax = max(LOWQ_CN)
    fcw = rng.integers(INT32_MIN, 1 << 31, Cmax).astype(np.int64)
    fcw[1] = INT32_MIN
    src = HOP_SRC[:Cmax]
    taps1 = (rng.standard_normal(L1) / np.sqrt(L1)).astype(np.float32)
    taps2 = (rng.standard_normal(L2) / np.sqrt(L2)).astype(np.float32)
    gain = GAINS[1]
    exp = np.stack([w2.tune2(host[src[c]][: Tmax * R], taps1, R1, taps2, R2, int(fcw[c]), gain) for c in range(Cmax)])
    if f == wl.IQ_F32:
        assert np.isnan(exp[BAD_SRC]).any() and np.isfinite(exp[0]).all()
    ctx = m17hip.Context(Cmax, Tmax)
    try:
        assert _config2(ctx, HOP_S, R1, taps1, R2, taps2, f) == 0
        ctx.wide_channels(src, fcw)
        for T in LOWQ_TS:
            for Cn in LOWQ_CN:
                ctx.reset()   # (a fresh feed: every T is a prefix of the one expectation)
                assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), Cn, T, P, gain) == 0
                ctx.C, ctx.T = Cn, T
                _assert_words(ctx.download_f32(), exp[:Cn, :T], (case, fmt, Cn, T))
    finally:
        ctx.close()


# ---- 2: the feed ---------------------------------------------------------------------------------------------------------------------------------
# (10, 5, 81, 161): a block of one output is 50 samples against a history of 1680; (16, 1, 129, 33): 16 against 640
FEED_CASES = [(10, 5, 81, 161), (16, 1, 129, 33)]
FEED_S, FEED_C = 2, 5
FEED_LENS = (1, 2, 255, 1, 300, 3, 200)   # outputs per block
FEED_CUTS = np.cumsum((0,) + FEED_LENS).tolist()
FEED_T = FEED_CUTS[-1]
FEED_SRC = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
FEED_HZ = (12500.0, -75000.0, 0.0, 101000.0, -3000.0)
FEED_GAIN = 1.25


def _feed_case(case, seed=6105, outputs=FEED_T):
    R1, R2, L1, L2 = case
    R = R1 * R2
    rng = np.random.default_rng(seed + R)
    x = rng.integers(-20000, 20001, size=(FEED_S, outputs * R, 2)).astype(np.int16)
    taps1 = (rng.standard_normal(L1) / np.sqrt(L1)).astype(np.float32)
    taps2 = (rng.standard_normal(L2) / np.sqrt(L2)).astype(np.float32)
    fcw = np.array([m17hip.wide_fcw(h, R) for h in FEED_HZ], dtype=np.int64)
    x.setflags(write=False)
    return x, taps1, taps2, fcw


@pytest.mark.parametrize("case", FEED_CASES, ids=["10x5", "16x1"])
def test_two_stage_blocks_continue_one_another_across_the_main_and_the_copy_stream(case):
    """Blocks of 1, 2, 255, 1, 300, 3 and 200 outputs — in place from device memory, staged from device and from pinned memory, and through the host form by
    turns: each finds the sources' histories and the channels' carries the block before it left, whichever stream that ran on.  Checked block by block
    against the host form fed the same blocks, and the concatenation is the one-block result."""
    import torch
    R1, R2, L1, L2 = case
    R = R1 * R2
    x, taps1, taps2, fcw = _feed_case(case)
    whole = w2.tune2_channels(x, FEED_SRC, fcw, taps1, R1, taps2, R2, FEED_GAIN)
    ref = w2.Feeds2(x, taps1, R1, taps2, R2, FEED_SRC, fcw, FEED_GAIN)
    dev = _dev(x)
    pin = torch.from_numpy(np.array(x)).pin_memory()
    sb, W = SB[wl.IQ_I16], FEED_T * R
    assert w2.hist_len(L1, R1, L2) > 30 * R   # (the short blocks are far shorter than the history)
    ctx = m17hip.Context(FEED_C, max(FEED_LENS))
    try:
        ctx.wide_config2(FEED_S, R1, R2, wl.IQ_I16, taps1, taps2)
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()
        how = ["in_place", "staged_device", "host", "staged_pinned", "staged_device", "in_place", "staged_pinned"]
        for (a, b), h in zip(zip(FEED_CUTS[:-1], FEED_CUTS[1:]), how):
            off = a * R * sb
            if h == "in_place":
                ctx.upload_wide_device(dev.data_ptr() + off, FEED_C, b - a, W, FEED_GAIN)
            elif h == "host":
                ctx.upload_wide(x[:, a * R: b * R], gain=FEED_GAIN)
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


def test_table_changes_resets_and_the_two_configurations_replacing_one_another():
    case = FEED_CASES[0]
    R1, R2, L1, L2 = case
    R = R1 * R2
    T = 192   # (m17hip_demod_reset_channels wants the context's position on the tick grid)
    x, taps1, taps2, fcw = _feed_case(case, seed=6106, outputs=9 * T)
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], 9 * T * R
    ctx = m17hip.Context(FEED_C, T * R2)
    ref = w2.Feeds2(x, taps1, R1, taps2, R2, FEED_SRC, fcw, FEED_GAIN)
    try:
        ctx.wide_config2(FEED_S, R1, R2, wl.IQ_I16, taps1, taps2)
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()

        def up(k, staged=False, n=T):
            getattr(ctx, "upload_wide_device_async" if staged else "upload_wide_device")(dev.data_ptr() + k * T * R * sb, FEED_C, n, W, FEED_GAIN)

        up(0)
        _assert_words(ctx.download_f32(), ref.block(0, T), "block 0")
        # a retune between blocks: channel 0 to another offset, channel 1 to the other source; the first output behind it is one sample of mismatch, nothing more
        old = w2.Feeds2(x, taps1, R1, taps2, R2, FEED_SRC, fcw, FEED_GAIN)
        old.block(0, T)
        ctx.wide_channels([0, 0], [m17hip.wide_fcw(-400000.0, R), fcw[1]])
        ref.src[1], ref.fcw[0] = 0, m17hip.wide_fcw(-400000.0, R)
        up(1)
        e1, o1 = ref.block(T, 2 * T), old.block(T, 2 * T)
        assert not np.array_equal(_u32(e1[:2]), _u32(o1[:2])) and np.array_equal(_u32(e1[2:]), _u32(o1[2:]))
        fresh = w2.tune2_channels(x, ref.src[:2], ref.fcw[:2], taps1, R1, taps2, R2, FEED_GAIN)[:, T:2 * T]   # (on the new table from the feed's beginning)
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
        f5 = w2.Feeds2(x[:, 5 * T * R:], taps1, R1, taps2, R2, ref.src, ref.fcw, FEED_GAIN)
        e5 = f5.block(0, T)
        assert not np.array_equal(_u32(e5), _u32(ref.block(5 * T, 6 * T)))
        _assert_words(ctx.download_f32(), e5, "block 5, after reset")
        # wide_config2 again starts the sources over and leaves the carries
        assert _config2(ctx, FEED_S, R1, taps1, R2, taps2, wl.IQ_I16) == 0
        up(6)
        f6 = w2.Feeds2(x[:, 6 * T * R:], taps1, R1, taps2, R2, ref.src, ref.fcw, FEED_GAIN)
        f6.carry = [c.copy() for c in f5.carry]
        _assert_words(ctx.download_f32(), f6.block(0, T), "block 6, after a second wide_config2")
        # wide_config takes over: the single-stage tuner at decim1 with the first stage's taps, wide_lib.Tuner's words (rows of n * decim1 samples; the
        # frequency words now mean fcw / 2^32 * 48000 * decim1 Hz), the carries still the channels' last z
        ctx.timing(True)
        assert g1._config(ctx, FEED_S, R1, wl.IQ_I16, taps1) == 0
        n1 = T * R2   # (the same samples per source)
        up(7, n=n1)
        f7 = wl.Feeds(x[:, 7 * T * R:], taps1, ref.src, ref.fcw, R1, FEED_GAIN)
        f7.carry = [c.copy() for c in f6.carry]
        ctx.C, ctx.T = FEED_C, n1
        _assert_words(ctx.download_f32(), f7.block(0, n1), "block 7, after wide_config")
        assert ctx.timing_get("tune")[1] == 1 and ctx.timing_get("tune2")[1] == 0
        # ... and wide_config2 again: the two-stage tuner, from a fresh feed of the sources
        assert _config2(ctx, FEED_S, R1, taps1, R2, taps2, wl.IQ_I16) == 0
        up(8)
        f8 = w2.Feeds2(x[:, 8 * T * R:], taps1, R1, taps2, R2, ref.src, ref.fcw, FEED_GAIN)
        f8.carry = [c.copy() for c in f7.carry]
        ctx.C, ctx.T = FEED_C, T
        _assert_words(ctx.download_f32(), f8.block(0, T), "block 8, after wide_config2 again")
        assert ctx.timing_get("tune")[1] == 1 and ctx.timing_get("tune2")[1] == 1
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 3: the full chain at 10 x 5 -----------------------------------------------------------------------------------------------------------------
CH_R1, CH_R2 = 10, 5
CH_R = CH_R1 * CH_R2
CH_OFFSETS = (-762500.0, 12500.0, 25000.0)   # tests/test_wide2_input.py's: one 12.5 kHz from its neighbour, one beyond any single-stage source
CH_SIGMA = 300.0 * np.sqrt(10.0)
CH_KINDS = (1, 2, 4)
CH_C = 6   # channels 0..2: the three transmissions on source 0; 3..5: the same on source 1 — the spectrum flipped — at the mirrored offsets, inverted


@pytest.fixture(scope="module")
def chain_case():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in CH_KINDS]
    x0 = wl.wideband(bb, CH_OFFSETS, CH_R, amplitude=6000.0, sigma=CH_SIGMA, seed=1, fmt=wl.IQ_I16)
    x = np.stack([x0, x0 * np.array([1, -1], dtype=np.int16)])
    src = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint32)
    fcw = np.array([m17hip.wide_fcw(f, CH_R) for f in CH_OFFSETS] + [m17hip.wide_fcw(-f, CH_R) for f in CH_OFFSETS], dtype=np.int64)
    pol = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8)
    taps1, taps2 = m17hip.wide_default_taps2(CH_R1, CH_R2)
    y = w2.tune2_channels(x, src, fcw, taps1, CH_R1, taps2, CH_R2, 1.0)
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
        ctx.wide_config2(2, CH_R1, CH_R2)   # (int16, the default taps of both stages)
        ctx.wide_channels(src, fcw)
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_wide(x if src_kind == "host" else _dev(x))
        _assert_words(ctx.download_f32(), y, src_kind)
        ctx.run()
        rows, logs = exp.run(0, T)
        g1._check(ctx, rows, logs, src_kind, cap, diags=exp.diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
def test_full_chain_pipelined_in_ragged_segments(chain_case, order):
    """A live feed: m17hip_upload_wide_device_async of segment k + 1, m17hip_demod_front, run — the two-stage tuner of the next segment on the copy stream
    beside the state-machine half of the current run; segments of ragged multiples of 192, mixed polarity."""
    x, src, fcw, pol, y, exp = chain_case
    T = y.shape[1]
    b = [0, 192, 192 * 27, 192 * 28, 192 * 75, 192 * 120, T]
    lens = [b1 - b0 for b0, b1 in zip(b[:-1], b[1:])]
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(CH_C, max(lens))
    try:
        ctx.wide_config2(2, CH_R1, CH_R2)
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
            g1._check(ctx, rows, None, f"pipelined {order}, segment {k}", 0, diags=None if more else exp.diags, got=got)
            if more and order != "run_then_fetch":
                ctx.run(channels=CH_C, samples=lens[k + 1])
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


# ---- 4: state rules ------------------------------------------------------------------------------------------------------------------------------
NAMES = g1.NAMES


def test_state_rules_refusals_memory_and_timing():
    import torch
    case = FEED_CASES[0]
    R1, R2, L1, L2 = case
    R = R1 * R2
    x, taps1, taps2, fcw = _feed_case(case)
    whole = w2.tune2_channels(x, FEED_SRC, fcw, taps1, R1, taps2, R2, FEED_GAIN)
    Cn, T = FEED_C, 384
    xi = np.ascontiguousarray(x[:, : T * R])
    dev, pin = _dev(xi), torch.from_numpy(xi.copy()).pin_memory()
    ptrs = dict(zip(NAMES, (xi.ctypes.data, pin.data_ptr(), dev.data_ptr(), dev.data_ptr())))
    maxC = Cn + 2
    ctx = m17hip.Context(maxC, T)
    try:
        assert ctx.iq_bytes() == 0
        for name in NAMES:   # before any configuration
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        # every refusal of wide_config2: each limit from outside, NULL / 0 combinations, a non-finite tap in either stage
        one, t256, t1024 = np.ones(1, dtype=np.float32), np.ones(256, dtype=np.float32), np.ones(1024, dtype=np.float32)
        bad = np.array([1.0, np.nan], dtype=np.float32)

        def cfg(S, d1, t1, n1, d2, t2, n2, fm):
            return ctx.lib.m17hip_wide_config2(ctx.h, C.c_uint32(S), C.c_uint32(d1), None if t1 is None else ol._p(t1), C.c_uint32(n1), C.c_uint32(d2),
                                               None if t2 is None else ol._p(t2), C.c_uint32(n2), C.c_int(fm))

        for args in ((0, 10, one, 1, 5, one, 1, 1), (257, 10, one, 1, 5, one, 1, 1), (1, 0, one, 1, 5, one, 1, 1), (1, 17, one, 1, 5, one, 1, 1),
                     (1, 10, one, 1, 0, one, 1, 1), (1, 10, one, 1, 17, one, 1, 1), (1, 10, one, 1, 5, one, 1, 0), (1, 10, one, 1, 5, one, 1, 4),
                     (1, 10, one, 0, 5, one, 1, 1), (1, 10, None, 1, 5, one, 1, 1), (1, 10, one, 1, 5, one, 0, 1), (1, 10, one, 1, 5, None, 1, 1),
                     (1, 10, np.ones(257, dtype=np.float32), 257, 5, one, 1, 1), (1, 10, one, 1, 5, np.ones(1025, dtype=np.float32), 1025, 1),
                     (1, 10, bad, 2, 5, one, 1, 1), (1, 10, one, 1, 5, bad, 2, 1), (1, 10, np.array([np.inf], dtype=np.float32), 1, 5, one, 1, 1)):
            assert cfg(*args) == EINVAL, args[:2] + args[3:5] + args[6:]
        assert ctx.iq_bytes() == 0
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        # the limits themselves, from inside
        assert cfg(256, 16, t256, 256, 16, t1024, 1024, 3) == 0
        assert cfg(1, 1, one, 1, 1, one, 1, 1) == 0
        assert cfg(1, 10, None, 0, 5, None, 0, 2) == 0 and cfg(1, 10, one, 1, 5, None, 0, 2) == 0 and cfg(1, 10, None, 0, 5, one, 1, 2) == 0
        # memory: the carry; both stages' taps, two histories and the z of a launch
        ctx.wide_config2(FEED_S, R1, R2, wl.IQ_I16, taps1, taps2)
        H = w2.hist_len(L1, R1, L2)
        held = ctx.iq_bytes()
        assert held == maxC * 8 + (L1 + L2) * 4 + 2 * FEED_S * H * 8 + maxC * 8
        g1._config(ctx, FEED_S, R1, wl.IQ_I16, taps1)
        assert ctx.iq_bytes() == maxC * 8 + L1 * 4 + 2 * FEED_S * (L1 - 1) * 8 + maxC * 8, "wide_config gives the second stage's memory back"
        ctx.wide_config2(FEED_S, R1, R2, wl.IQ_I16, taps1, taps2)
        assert ctx.iq_bytes() == held
        ctx.wide_channels(FEED_SRC, fcw)
        ctx.reset()
        # timing index 10 counts this tuner's launches, index 9 does not
        ctx.timing(True)
        ctx.upload_wide_device(dev.data_ptr(), Cn, T, T * R, FEED_GAIN)
        assert ctx.iq_bytes() == held + 2 * maxC * 4, "the device forms add one copy of the channel table"
        _assert_words(ctx.download_f32(), whole[:, :T], "device")
        ctx.reset()
        ctx.upload_wide(xi, gain=FEED_GAIN, channels=Cn)
        assert ctx.iq_bytes() == held + 2 * maxC * 4 + FEED_S * T * R * 4, "and the host forms the raw block"
        _assert_words(ctx.download_f32(), whole[:, :T], "host")
        ms, launches = ctx.timing_get("tune2")
        assert launches == 2 and ms > 0, "one launch per block"
        assert ctx.timing_get("tune")[1] == 0 and ctx.timing_get("discriminate")[1] == 0
        ctx.timing(False)
        # the argument refusals, every way in: a pitch shorter than samples * decim1 * decim2 among them (one that would do for a single stage too)
        for name in NAMES:
            p = ptrs[name]
            assert _raw(ctx, name, None, Cn, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, 0, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, 0, T * R) == EINVAL, name
            assert _raw(ctx, name, p, maxC + 1, T, T * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T + 1, (T + 1) * R) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T, T * R - 1) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T, T * R1) == EINVAL, name
            assert _raw(ctx, name, p, Cn, T, T * R, float("nan")) == EINVAL, name
        # between m17hip_demod_front and its run the slabs are the run's — and so is the configuration
        ctx.run()
        ctx.upload_wide_device_async(dev.data_ptr(), Cn, T, T * R)
        ctx.front(channels=Cn, samples=T)
        for name in NAMES:
            assert _raw(ctx, name, ptrs[name], Cn, T, T * R) == ESTATE, name
        assert _config2(ctx, FEED_S, R1, taps1, R2, taps2, wl.IQ_I16) == ESTATE
        ctx.run(channels=Cn, samples=T)
        ctx.upload_wait()
        ctx.frames()
    finally:
        ctx.close()


def test_a_row_of_2_to_the_32_samples_is_refused():
    """16 777 216 outputs at 16 x 16 are 2^32 complex samples per row: the kernels count a row's samples in 32 bits.  Refused on the arguments alone, before
    the pointer is looked at, whatever the pitch; at 15 x 16 the same block is 2^32 - 2^28 samples and the refusal is only the pitch's."""
    T = 1 << 24
    ctx = m17hip.Context(1, T)
    one = np.ones(1, dtype=np.float32)
    dummy = np.zeros(16, dtype=np.int16)
    try:
        assert _config2(ctx, 1, 16, one, 16, one, wl.IQ_I16) == 0
        for name in NAMES:
            assert _raw(ctx, name, dummy.ctypes.data, 1, T, 1 << 32) == EINVAL, name
            assert _raw(ctx, name, dummy.ctypes.data, 1, T, 1 << 33) == EINVAL, name
        assert _config2(ctx, 1, 15, one, 16, one, wl.IQ_I16) == 0
        assert _raw(ctx, NAMES[0], dummy.ctypes.data, 1, T, (1 << 32) - (1 << 28) - 1) == EINVAL
    finally:
        ctx.close()


# ---- 5: the example ------------------------------------------------------------------------------------------------------------------------------
def test_example_tunes_a_2400k_source_on_the_device(chain_case):
    """examples/m17-demod-gpu --wide-i16 --decim 10 --decim2 5 --offset-hz 12500: M17Demodulator<float>::wide buffers the wideband and uploads it block by
    block (m17hip_wide_config2, the feed carried on the device); its frame callbacks are the float oracle's on the host form's floats, in order."""
    x, src, fcw, pol, y, exp = chain_case
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe, "--wide-i16", "--decim", "10", "--decim2", "5", "--offset-hz", "12500"], input=np.ascontiguousarray(x[0]).tobytes(),
                         capture_output=True, check=True, timeout=120).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    recs, _ = fl.demod(y[1])
    e = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == e and len(e) >= 6
