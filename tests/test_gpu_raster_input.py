"""GPU tests of wideband IQ input on a channel raster (ABI 611, include/m17hip.h: m17hip_wide_raster): chan_kernel folds each source's samples once per
output time, takes the DFT in two passes and discriminates the bins that channels listen to into the float input slab.  Every comparison is exact: the
floats (m17hip_download_f32) as uint32 words against the HOST form of the same arithmetic (tests/cxx/raster_oracle.cpp: detail/core.h's chan_fold /
chan_pass1 / chan_pass2 under the host compiler, over the twiddle table the library exports) — NaN-ness where that is a NaN — and records, m17_diag and the
diagnostic log byte for byte against the float oracle stepped on the host form's floats.  What the host form itself is worth is asserted without a GPU in
tests/test_raster_input.py.  The helpers of tests/test_gpu_wide_input.py are imported as they stand."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import raster_lib as rl
import test_gpu_wide_count_wrap as wrap
import test_gpu_wide_input as g1
import wide2_lib as w2
import wide_lib as wl
from test_gpu_wide_count_wrap import big   # noqa: F401  (the reused 512 MB device buffer, a fixture)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS, SB, GAINS = g1.FMTS, g1.SB, g1.GAINS
_u32, _assert_words, _dev, _raw = g1._u32, g1._assert_words, g1._dev, g1._raw


def _raster(ctx, S, R, M, fmt, taps):
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    return ctx.lib.m17hip_wide_raster(ctx.h, C.c_uint32(S), C.c_uint32(R), C.c_uint32(M), C.c_int(fmt), None if t is None else ol._p(t),
                                      C.c_uint32(0 if t is None else t.size))


def _channels(ctx, src, bins):
    s, b = np.ascontiguousarray(src, dtype=np.uint32), np.ascontiguousarray(bins, dtype=np.int32)
    return ctx.lib.m17hip_wide_raster_channels(ctx.h, ol._p(s), ol._p(b), C.c_uint32(s.size))


def _data(fmt, S, P, rng, bad=None):
    """S source rows of P samples: full-range integers with both rails and a zero; floats up to 1e9 with denormals and zeroes, and in source `bad`
    infinities and NaNs."""
    if fmt == wl.IQ_I16:
        x = rng.integers(-32768, 32768, size=(S, P, 2)).astype(np.int16)
        x[:, 5 % P] = (-32768, 32767)
        x[:, 9 % P] = 0
    elif fmt == wl.IQ_U8:
        x = rng.integers(0, 256, size=(S, P, 2)).astype(np.uint8)
        x[:, 5 % P] = (0, 255)
    else:
        x = (12000.0 * (rng.standard_normal((S, P)) + 1j * rng.standard_normal((S, P)))).astype(np.complex64)
        x = g1._spice(x, rng)
        if bad is not None:
            v = x[bad].view(np.float32)
            for k, val in zip(rng.choice(np.arange(40, 2 * P, 97), 6, replace=False), [np.inf, -np.inf, np.nan] * 2):
                v[k] = val
    x.setflags(write=False)
    return x


def _all_bins(M):
    return list(range(-(M // 2), (M - 1) // 2 + 1))


def _table(M, S, extra_rng):
    """Every bin of source 0, three of them once more (several channels on one bin), and a few bins of the last source — in a shuffled channel order."""
    bins = _all_bins(M)
    src = [0] * M
    bins += [bins[0], bins[-1], 1 % M if M > 2 else 0]
    src += [0] * 3
    if S > 1:
        few = [-(M // 2), 0, (M - 1) // 2, 1 if M > 2 else 0]
        bins += few
        src += [S - 1] * len(few)
    order = extra_rng.permutation(len(bins))
    return np.array(src, dtype=np.uint32)[order], np.array(bins, dtype=np.int32)[order]


def _hop(M, R, L, fmt, Ts, S, seed, taps=None, ways=("host", "device"), bad=None):
    rng = np.random.default_rng(seed)
    Tmax = max(Ts)
    P = Tmax * R + 3   # odd: rows are not 16-byte aligned (a sample is aligned to its own size, no more)
    host = _data(fmt, S, P, rng, bad)
    dev = _dev(host)
    if taps is None:
        taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    src, bins = _table(M, S, rng)
    Cmax = src.size
    exp = {g: rl.chan_channels([host[s][: Tmax * R] for s in range(S)], src, bins, taps, R, M, g) for g in GAINS}
    if bad is not None and fmt == wl.IQ_F32:
        e = exp[GAINS[0]]
        assert np.isnan(e[src == bad]).any() and np.isfinite(e[src != bad]).all()
    ctx = m17hip.Context(Cmax, Tmax)
    try:
        assert _raster(ctx, S, R, M, fmt, taps) == 0
        assert _channels(ctx, src, bins) == 0
        for ti, T in enumerate(Ts):
            for k, way in enumerate(ways):
                gain = GAINS[(ti + k) & 1]
                ctx.reset()   # (a fresh feed: histories, count and carries are zero)
                name, ptr = ("m17hip_upload_wide", host.ctypes.data) if way == "host" else ("m17hip_upload_wide_device", dev.data_ptr())
                assert _raw(ctx, name, ptr, Cmax, T, P, gain) == 0
                ctx.C, ctx.T = Cmax, T
                assert ctx.input_format()[0] == m17hip.FORMAT_F32
                _assert_words(ctx.download_f32(), exp[gain][:, :T], (M, R, L, fmt, T, gain, way))
    finally:
        ctx.close()


# ---- 1: one hop ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rl.SMALL, ids=["M{}_R{}_L{}".format(*s) for s in rl.SMALL])
def test_channeliser_small_shapes(shape):
    """The shapes where indexing can go wrong (tests/test_raster_input.py's), one output, a tile's edges and two tiles and three: the host form's words."""
    M, R, L = shape
    tt, lds = rl.tile_and_lds(L, R, M)
    assert tt == 31 and lds <= 65536
    _hop(M, R, L, wl.IQ_I16, (1, tt - 1, tt, tt + 1, 2 * tt + 3), 2, 6200 + M + R + L)


@pytest.mark.parametrize("fmt", list(FMTS), ids=list(FMTS))
def test_channeliser_192_bins_of_a_2400k_source(fmt):
    """M = 192, decim 50, the 1601 default taps, 300 outputs (23 tiles of 13 and one of 1), two sources: all 192 bins of source 0, three of them twice, and
    four bins of source 1 — which in float32 holds infinities and NaNs, staying in the channels that listen to it."""
    M, R = 192, 50
    taps = m17hip.wide_raster_default_taps(R)
    assert taps.size == 1601 and rl.tile_and_lds(1601, R, M)[0] == 13
    _hop(M, R, 1601, FMTS[fmt], (300,), 2, 6210 + FMTS[fmt], taps=taps, ways=("device",) if fmt != "i16" else ("host", "device"), bad=1)


def test_channeliser_at_the_limits_of_its_configuration():
    """M = 256, decim 64, 4096 taps: tiles of 5 outputs in 64 KB of LDS, and it must launch.  40 outputs and the tile's edges."""
    tt, lds = rl.tile_and_lds(4096, 64, 256)
    assert tt == 5 and lds <= 65536
    _hop(256, 64, 4096, wl.IQ_I16, (40, 1, tt - 1, tt, tt + 1), 2, 6220, ways=("device",))


def test_tile_edges_at_192_bins():
    M, R, L = 192, 50, 1601
    tt, lds = rl.tile_and_lds(L, R, M)
    assert lds <= 65536
    _hop(M, R, L, wl.IQ_U8, (1, tt - 1, tt, tt + 1), 1, 6230, ways=("device",))


def test_the_last_of_256_sources_and_a_channel_count_below_the_table():
    """256 sources of which only the last and the first are heard; then fewer channels than the table names: the rest of the slab's rows are not written
    by the launch and the listed ones are the host form's."""
    M, R, L, S, T = 12, 4, 5, 256, 40
    rng = np.random.default_rng(6240)
    x = _data(wl.IQ_U8, S, T * R, rng)
    taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    src, bins = np.array([255, 0, 255, 0], dtype=np.uint32), np.array([-6, 5, 0, 0], dtype=np.int32)
    exp = rl.chan_channels([x[s] for s in range(S)], src, bins, taps, R, M, 1.0)
    ctx = m17hip.Context(4, T)
    try:
        ctx.wide_raster(S, R, M, wl.IQ_U8, taps)
        ctx.wide_raster_channels(src, bins)
        ctx.reset()
        ctx.upload_wide(x)
        _assert_words(ctx.download_f32(), exp, "256 sources")
        for Cn in (1, 3):
            ctx.reset()
            ctx.upload_wide(x, channels=Cn)
            _assert_words(ctx.download_f32(), exp[:Cn], ("channels", Cn))
    finally:
        ctx.close()


# ---- 2: the feed ---------------------------------------------------------------------------------------------------------------------------------
FEED_M, FEED_R, FEED_L = 192, 50, 1601
FEED_S, FEED_C = 2, 6
FEED_LENS = (1, 2, 255, 1, 300, 3, 200)   # outputs per block: with decim 50 and M = 192 every boundary has another count mod M
FEED_CUTS = np.cumsum((0,) + FEED_LENS).tolist()
FEED_T = FEED_CUTS[-1]
FEED_SRC = np.array([0, 1, 1, 0, 1, 0], dtype=np.uint32)
FEED_BINS = np.array([1, -61, 0, 95, -96, 1], dtype=np.int32)   # (channels 0 and 5 on one bin of one source)
FEED_GAIN = 1.25


def _feed_case(seed=6250, outputs=FEED_T):
    rng = np.random.default_rng(seed)
    x = rng.integers(-20000, 20001, size=(FEED_S, outputs * FEED_R, 2)).astype(np.int16)
    taps = (rng.standard_normal(FEED_L) / np.sqrt(FEED_L)).astype(np.float32)
    x.setflags(write=False)
    return x, taps


def test_ragged_blocks_continue_one_another_across_the_main_and_the_copy_stream():
    """Blocks of 1, 2, 255, 1, 300, 3 and 200 outputs — in place from device memory, staged from device and from pinned memory, and through the host form
    by turns: each finds the sources' histories, the count and the channels' carries the block before it left, whichever stream that ran on.  Checked block
    by block against the host form fed the same blocks, and the concatenation is the one-block result."""
    import torch
    x, taps = _feed_case()
    R = FEED_R
    assert len({(a * R) % FEED_M for a in FEED_CUTS[:-1]}) == len(FEED_CUTS) - 1
    whole = rl.chan_channels(x, FEED_SRC, FEED_BINS, taps, R, FEED_M, FEED_GAIN)
    ref = rl.Feeds(x, taps, R, FEED_M, FEED_SRC, FEED_BINS, FEED_GAIN)
    dev = _dev(x)
    pin = torch.from_numpy(np.array(x)).pin_memory()
    sb, W = SB[wl.IQ_I16], FEED_T * R
    ctx = m17hip.Context(FEED_C, max(FEED_LENS))
    try:
        ctx.wide_raster(FEED_S, R, FEED_M, wl.IQ_I16, taps)
        ctx.wide_raster_channels(FEED_SRC, FEED_BINS)
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
            _assert_words(ctx.download_f32(), e, (h, a, b))
        ctx.upload_wait()
    finally:
        ctx.close()


def test_table_changes_a_staged_block_resets_and_the_configurations_replacing_one_another():
    T = 192   # (m17hip_demod_reset_channels wants the context's position on the tick grid)
    R, M = FEED_R, FEED_M
    x, taps = _feed_case(seed=6251, outputs=9 * T)
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], 9 * T * R
    ctx = m17hip.Context(FEED_C, T * 5)
    ref = rl.Feeds(x, taps, R, M, FEED_SRC, FEED_BINS, FEED_GAIN)
    try:
        ctx.timing(True)
        ctx.wide_raster(FEED_S, R, M, wl.IQ_I16, taps)
        ctx.wide_raster_channels(FEED_SRC, FEED_BINS)
        ctx.reset()

        def up(k, staged=False, n=T):
            getattr(ctx, "upload_wide_device_async" if staged else "upload_wide_device")(dev.data_ptr() + k * T * R * sb, FEED_C, n, W, FEED_GAIN)

        up(0)
        _assert_words(ctx.download_f32(), ref.block(0, T), "block 0")
        # a retune between blocks: channel 0 to another bin, channel 1 to the other source; the tuners' table call is not this configuration's
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.zeros(1, dtype=np.uint32)), ol._p(np.zeros(1, dtype=np.int32)), C.c_uint32(1)) == ESTATE
        ctx.wide_raster_channels([0, 0], [-30, int(FEED_BINS[1])])
        ref.src[1], ref.bins[0] = 0, -30
        up(1)
        _assert_words(ctx.download_f32(), ref.block(T, 2 * T), "block 1, retuned")
        # a staged block beside a run keeps the table it was tuned with: the change behind it applies from the block after
        up(2, staged=True)
        ctx.front(channels=FEED_C, samples=T)
        assert _channels(ctx, [1], [7]) == 0   # (never waits, and is no configuration call: allowed between front and run)
        assert _raster(ctx, FEED_S, R, M, wl.IQ_I16, taps) == ESTATE
        e2 = ref.block(2 * T, 3 * T)
        ref.src[0], ref.bins[0] = 1, 7
        ctx.run(channels=FEED_C, samples=T)
        _assert_words(ctx.download_f32(), e2, "block 2, staged before the change")
        up(3)
        _assert_words(ctx.download_f32(), ref.block(3 * T, 4 * T), "block 3, after the change")
        # reset_channels: the listed channels' carries are zero at once; nothing else changes
        ctx.reset_channels([1, 3])
        ref.carry[[1, 3]] = 0
        up(4)
        e4 = ref.block(4 * T, 5 * T)
        assert (e4[[1, 3], 0] == 0).all() and (e4[[0, 2, 4, 5], 0] != 0).all()
        _assert_words(ctx.download_f32(), e4, "block 4, two carries zeroed")
        # demod_reset: count, histories and carries start over — a fresh host form on the same table
        ctx.reset()
        up(5)
        f5 = rl.Feeds(x[:, 5 * T * R:], taps, R, M, ref.src, ref.bins, FEED_GAIN)
        e5 = f5.block(0, T)
        assert not np.array_equal(_u32(e5), _u32(ref.block(5 * T, 6 * T)))
        _assert_words(ctx.download_f32(), e5, "block 5, after reset")
        assert ctx.timing_get("channelise")[1] == 6 and ctx.timing_get("tune2")[1] == 0 and ctx.timing_get("tune")[1] == 0
        # wide_config2 takes over: the two-stage tuner at 10 x 5 on a fresh table (a bin is no frequency word), the carries still the channels' last z
        ctx.wide_config2(FEED_S, 10, 5, wl.IQ_I16)
        assert _channels(ctx, [0], [0]) == ESTATE
        fcw = [m17hip.wide_fcw(12500.0 * b, R) for b in (1, -61, 0, 95, -96, 1)]
        ctx.wide_channels(FEED_SRC, fcw)
        up(6)
        t1, t2 = m17hip.wide_default_taps2(10, 5)
        f6 = w2.Feeds2(x[:, 6 * T * R:], t1, 10, t2, 5, FEED_SRC, fcw, FEED_GAIN)
        f6.carry = [c.copy() for c in f5.carry]
        _assert_words(ctx.download_f32(), f6.block(0, T), "block 6, after wide_config2")
        assert ctx.timing_get("channelise")[1] == 6 and ctx.timing_get("tune2")[1] == 1
        # ... and the raster again: every channel back on (source 0, bin 0) until the table is written, from a fresh feed of the sources
        ctx.wide_raster(FEED_S, R, M, wl.IQ_I16, taps)
        up(7)
        f7 = rl.Feeds(x[:, 7 * T * R:], taps, R, M, [0] * FEED_C, [0] * FEED_C, FEED_GAIN)
        f7.carry[:] = np.stack(f6.carry)
        _assert_words(ctx.download_f32(), f7.block(0, T), "block 7, the raster again with a fresh table")
        ctx.wide_raster_channels(FEED_SRC, FEED_BINS)
        f7.src, f7.bins = list(FEED_SRC), list(FEED_BINS)
        up(8)
        _assert_words(ctx.download_f32(), f7.block(T, 2 * T), "block 8")
        assert ctx.timing_get("channelise")[1] == 8
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 3: the full chain on a 2.4 MSPS source ------------------------------------------------------------------------------------------------------
CH_R, CH_M = 50, 192
CH_BINS = (-61, 1, 2)   # -762.5, +12.5 and +25 kHz: tests/test_wide2_input.py's transmissions
CH_SIGMA = 300.0 * np.sqrt(10.0)
CH_KINDS = (1, 2, 4)
CH_C = 6   # channels 0..2: the three transmissions on source 0; 3..5: the same on source 1 — the spectrum flipped — at the mirrored bins, inverted


@pytest.fixture(scope="module")
def chain_case():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in CH_KINDS]
    x0 = wl.wideband(bb, [12500.0 * b for b in CH_BINS], CH_R, amplitude=6000.0, sigma=CH_SIGMA, seed=1, fmt=wl.IQ_I16)
    x = np.stack([x0, x0 * np.array([1, -1], dtype=np.int16)])
    src = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint32)
    bins = np.array(list(CH_BINS) + [-b for b in CH_BINS], dtype=np.int32)
    pol = np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8)
    y = rl.chan_channels(x, src, bins, m17hip.wide_raster_default_taps(CH_R), CH_R, CH_M, 1.0)
    exp = g1.Expect(y, invert=pol)
    good = [r[(r["cost"] < 30) & (r["frame_type"] != 1)] for r in exp.recs]
    assert all(g.size >= 7 for g in good), "every channel yields its transmission's frames"
    for c in range(3):
        assert good[c]["payload"].tobytes() == good[c + 3]["payload"].tobytes()
    for a in (x, y):
        a.setflags(write=False)
    return x, src, bins, pol, y, exp


@pytest.mark.parametrize("src_kind", ["host", "tensor"])
def test_full_chain_in_one_run(chain_case, src_kind):
    x, src, bins, pol, y, exp = chain_case
    T = y.shape[1]
    cap = T // 384 + 2
    ctx = m17hip.Context(CH_C, T)
    try:
        ctx.tune(9, cap)
        ctx.wide_raster(2, CH_R, CH_M)   # (int16, the default taps)
        ctx.wide_raster_channels(src, bins)
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_wide(x if src_kind == "host" else _dev(x))
        _assert_words(ctx.download_f32(), y, src_kind)
        ctx.run()
        rows, logs = exp.run(0, T)
        g1._check(ctx, rows, logs, src_kind, cap, diags=exp.diags)
    finally:
        ctx.close()


def test_full_chain_pipelined_in_ragged_segments(chain_case):
    """A live feed: m17hip_upload_wide_device_async of segment k + 1, m17hip_demod_front, run, m17hip_frames_fetch — the channeliser of the next segment
    on the copy stream beside the state-machine half of the current run; segments of ragged multiples of 192, mixed polarity."""
    x, src, bins, pol, y, exp = chain_case
    T = y.shape[1]
    b = [0, 192, 192 * 27, 192 * 28, 192 * 75, 192 * 120, T]
    lens = [b1 - b0 for b0, b1 in zip(b[:-1], b[1:])]
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(CH_C, max(lens))
    try:
        ctx.wide_raster(2, CH_R, CH_M)
        ctx.wide_raster_channels(src, bins)
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
            got = ctx.frames().copy()
            ctx.frames_select(0)
            rows, _ = exp.run(b[k], b[k + 1])
            g1._check(ctx, rows, None, f"pipelined, segment {k}", 0, diags=None if more else exp.diags, got=got)
            if more:
                ctx.run(channels=CH_C, samples=lens[k + 1])
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


def test_example_channelises_on_the_device(chain_case):
    """examples/m17-demod-gpu --wide-i16 --decim 50 --raster 192 --bin 1: M17Demodulator<float>::wide buffers the wideband and uploads it block by block
    (m17hip_wide_raster, m17hip_upload_wide, the feed carried on the device); its frame callbacks are the float oracle's on the host form's floats."""
    import os
    import subprocess
    import f32_lib as fl
    import iq_lib as iq
    x, src, bins, pol, y, exp = chain_case
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe, "--wide-i16", "--decim", "50", "--raster", "192", "--bin", "1"], input=np.ascontiguousarray(x[0]).tobytes(), capture_output=True,
                         check=True, timeout=120).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    recs, _ = fl.demod(y[1])
    e = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == e and len(e) >= 6


# ---- 4: refusals, memory ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was_and_memory_is_counted():
    M, R, L, T = 12, 4, 5, 64
    rng = np.random.default_rng(6260)
    x = _data(wl.IQ_I16, 2, T * R, rng)
    dev = _dev(x)
    taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    src, bins = np.array([0, 1, 1], dtype=np.uint32), np.array([-6, 5, 0], dtype=np.int32)
    exp = rl.chan_channels(x, src, bins, taps, R, M, 1.0)
    ctx = m17hip.Context(3, T)
    try:
        assert ctx.iq_bytes() == 0
        assert _channels(ctx, src, bins) == ESTATE   # before any configuration
        ctx.wide_raster(2, R, M, wl.IQ_I16, taps)
        assert _channels(ctx, src, bins) == 0
        before = ctx.iq_bytes()
        assert before >= 8 * M + 4 * L + 2 * 8 * 2 * (L - 1)   # twiddles, taps, two histories of two sources
        one, big_t = np.ones(1, dtype=np.float32), np.ones(4097, dtype=np.float32)
        bad = np.array([1.0, np.inf], dtype=np.float32)
        for S_, R_, M_, f_, t_ in ((0, R, M, 1, taps), (257, R, M, 1, taps), (2, 0, M, 1, taps), (2, 65, M, 1, taps), (2, R, 0, 1, taps), (2, R, 34, 1, taps),
                                   (2, R, 17, 1, taps), (2, R, 257, 1, taps), (2, R, 512, 1, taps), (2, R, M, 0, taps), (2, R, M, 4, taps), (2, R, M, 1, big_t),
                                   (2, R, M, 1, bad)):
            assert _raster(ctx, S_, R_, M_, f_, t_) == EINVAL, (S_, R_, M_, f_)
        lib = ctx.lib
        assert lib.m17hip_wide_raster(ctx.h, C.c_uint32(2), C.c_uint32(R), C.c_uint32(M), C.c_int(1), None, C.c_uint32(3)) == EINVAL
        assert lib.m17hip_wide_raster(ctx.h, C.c_uint32(2), C.c_uint32(R), C.c_uint32(M), C.c_int(1), ol._p(one), C.c_uint32(0)) == EINVAL
        for s_, b_ in (([0, 2, 0], [0, 0, 0]), ([0, 1, 1], [6, 0, 0]), ([0, 1, 1], [0, 0, -7])):   # a source that is not there; a bin outside [-6, 6)
            assert _channels(ctx, s_, b_) == EINVAL
        assert lib.m17hip_wide_raster_channels(ctx.h, None, None, C.c_uint32(1)) == EINVAL
        assert _channels(ctx, [0] * 4, [0] * 4) == EINVAL   # more than the context's channels
        ctx.reset()
        assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), 3, T, T * R - 1) == EINVAL   # pitch below samples * decim
        assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), 3, T, T * R) == 0
        ctx.C, ctx.T = 3, T
        _assert_words(ctx.download_f32(), exp, "after the refusals")   # (configuration, table and feed are as they were)
        assert ctx.iq_bytes() >= before
        with pytest.raises(TypeError):
            ctx.upload_wide(np.zeros((2, T * R + 1, 2), dtype=np.int16))
        # the limits themselves are served, and the default taps are taken
        assert _raster(ctx, 256, 64, 256, wl.IQ_U8, np.ones(4096, dtype=np.float32)) == 0
        assert _raster(ctx, 1, 64, 13, wl.IQ_F32, None) == 0
    finally:
        ctx.close()


# ---- 5: the count across 2^32 ------------------------------------------------------------------------------------------------------------------------
class _OneBin:
    """raster_lib.Raster with one bin, in the shape tests/test_gpu_wide_count_wrap.py's _across steps a tuner."""

    def __init__(self, taps, R, M, b, count):
        self.r = rl.Raster(taps, R, M, [b], 1.0, count=count)
        self.hist = self.r.hist

    carry = property(lambda self: self.r.carry[0])
    count = property(lambda self: self.r.count)

    def block(self, row):
        return self.r.block(row)[0]


def test_channeliser_feed_across_2_to_the_32_samples(big):   # noqa: F811
    """One uint8 source, M = 192, decim 16, 33 taps, bin -61: sixteen in-place blocks of 2^28 samples, the last one 300 outputs short, then 1, 255 and 300
    outputs across the wrap against the host form started at that count.  2^32 mod 192 = 64: a count truncated to 32 bits jumps 64 bins at the wrap."""
    R, M, L, b = 16, 192, 33, -61
    assert (1 << 32) % M == 64
    taps = wl.hamming_taps(L)
    ctx = m17hip.Context(1, wrap.BIG // R)
    try:
        ctx.wide_raster(1, R, M, wl.IQ_U8, taps)
        ctx.wide_raster_channels([0], [b])
        ctx.reset()
        wrap._across(ctx, big, lambda count: _OneBin(taps, R, M, b, count), R, L - 1, wrap.BIG, "raster")
        # One block more, begun BEHIND the wrap: the count the host takes mod M is now above 2^32.  The host form's history and carry at this point come
        # from the tail of the blocks _across fed (its generator, restated), begun from zeroes that the last output no longer sees.
        n_cross, end = sum(wrap.CROSS), wrap.WRAP + (sum(wrap.CROSS) - wrap.BEFORE) * R
        fed = np.random.default_rng(6121 + R).integers(0, 256, size=(n_cross * R, 2)).astype(np.uint8)
        N = -(-(L - 1) // R) + 2
        t = _OneBin(taps, R, M, b, end - N * R)
        t.block(fed[-N * R:])
        assert t.count == end and end % M != (end & 0xFFFFFFFF) % M
        x = np.random.default_rng(6270).integers(0, 256, size=(50 * R, 2)).astype(np.uint8)
        ctx.upload_wide_device(_dev(x).data_ptr(), 1, 50, 50 * R)
        _assert_words(ctx.download_f32(), t.block(x)[None, :], "a block begun behind the wrap")
    finally:
        ctx.close()
