"""GPU tests of the sources' noise floor on the device (ABI 621, include/m17hip.h: m17hip_wide_squelch_floor): squelch_floor_kernel selects each source's
upper median from the block's own spectrum plane, tracks it and writes the levels the unchanged squelch kernels of both modes read.  Every comparison is exact
on uint32 words against the HOST form (tests/squelch_floor_lib.py over squelch_lib and squelch_slots_lib): floor planes, state words, bands, tile masks,
output slabs and meter planes; where the host form gives a NaN, a NaN.  What the host form itself is worth is asserted without a GPU in
tests/test_wide_squelch_floor.py.

The layout: 3 float32 sources, 8 channels, 64 points at hop 64.  Source 0 is noise with a carrier throughout (channels 0 and 1), one in blocks 0 and 3
(channel 2) and an empty bin (channel 3), and is 18 dB louder in block 2.  Source 1 is exact zeros (channels 4 and 5).  Source 2 is noise with a carrier
(channel 6) and an empty bin (channel 7) and holds an inf and a NaN sample in block 2.  Ratios 6 / 3 dB, rise 1 / 8, fall 1, hang 0."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import m17hip
import meter_lib as ml
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_floor_lib as sf
import squelch_lib as sq
import squelch_slots_lib as ssl
import test_gpu_wide_input as g1
import test_gpu_wide_squelch as g9
import test_gpu_wide_squelch_slots as gs
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
OPEN = sq.OPEN
NAN = sf.NAN
_u32, _assert_words, _dev = g1._u32, g1._assert_words, g1._dev
GAIN = g9.GAIN
POINTS, HOP, HALF = 64, 64, 1
RO, RC = m17hip.wide_squelch_ratio(6.0), m17hip.wide_squelch_ratio(3.0)
RISE, FALL = 0.125, 1.0
NBLOCKS = 4
F32 = wl.IQ_F32
SRC = [0, 0, 0, 0, 1, 1, 2, 2]
FCW = [10 << 26, 10 << 26, -(1 << 31), 20 << 26, 10 << 26, 20 << 26, (1 << 31) - 1, 20 << 26]
STRONG, SIGMA, LOUD = 5000.0, 20.0, 8.0
MODES = ("block", "slots")


class Kind:
    """One of the three tuners over 3 sources: T outputs per block of Wb samples in tiles of TO, configure(ctx, fmt, sources), tuner(fcw) -> its host form."""


def _kinds():
    out = {}
    k = Kind()
    k.T, k.Wb, k.TO = 1020, 5100, ssl.WIDE_TILE
    taps = m17hip.wide_default_taps(5)
    k.configure = lambda ctx, fmt, S=3: ctx.wide_config(S, 5, fmt)
    k.tuner = lambda w: wl.Tuner(taps, 5, w, GAIN)
    out["config"] = k
    k = Kind()
    k.T, k.Wb, k.TO = 1020, 4080, ssl.WIDE_TILE
    t1, t2 = m17hip.wide_default_taps2(2, 2)
    k.configure = lambda ctx, fmt, S=3: ctx.wide_config2(S, 2, 2, fmt)
    k.tuner = lambda w: w2.Tuner2(t1, 2, t2, 2, w, GAIN)
    out["config2"] = k
    k = Kind()
    r1, r2 = wl.hamming_taps(33), (3 * wl.hamming_taps(65).astype(np.float64)).astype(np.float32)   # (short taps: tests/test_resample_input.py's TILES)
    k.TO = rl.tile_outputs(r1.size, 16, r2.size, 3, 8)
    k.T = 2 * k.TO
    k.Wb = k.T // 3 * 8 * 16
    k.configure = lambda ctx, fmt, S=3: ctx.wide_resample(S, 16, 3, 8, fmt, r1, r2)
    k.tuner = lambda w: rl.Resampler(r1, 16, 3, 8, r2, w, GAIN)
    out["resample"] = k
    return out


KINDS = _kinds()


def _tone(x, s, word, a, b, ampl):
    n = np.arange(a, b)
    x[s, a:b] += ampl * np.exp(2j * np.pi * ((word * n) % (1 << 32)) / float(1 << 32))


@functools.lru_cache(maxsize=None)
def _source(kind):
    """data complex64 [3][NBLOCKS x Wb], read-only."""
    k = KINDS[kind]
    rng = np.random.default_rng(6210 + len(kind))
    W = NBLOCKS * k.Wb
    x = SIGMA * (rng.standard_normal((3, W)) + 1j * rng.standard_normal((3, W)))
    x[0, 2 * k.Wb:3 * k.Wb] *= LOUD
    x[1] = 0.0
    _tone(x, 0, FCW[0], 0, W, STRONG)
    _tone(x, 0, FCW[2], 0, k.Wb, STRONG)
    _tone(x, 0, FCW[2], 3 * k.Wb, W, STRONG)
    _tone(x, 2, FCW[6], 0, W, STRONG)
    data = x.astype(np.complex64)
    data[2, 2 * k.Wb + k.Wb // 3] = np.complex64(complex(np.inf, 1.0))
    data[2, 2 * k.Wb + k.Wb // 2] = np.complex64(complex(2.0, np.nan))
    data.setflags(write=False)
    return data


def _feed(kind, mode, data, fmin=0.0, src=SRC, fcw=FCW, sources=3, rise=RISE, fall=FALL):
    k = KINDS[kind]
    tuners = [k.tuner(w) for w in fcw]
    if mode == "block":
        feed = sf.Feed(tuners, src, data, POINTS, HOP)
        feed.squelch = sq.Squelch(src, fcw, np.ones(sources), np.ones(sources), HALF, 0)
    else:
        feed = sf.SlotFeed(tuners, src, data, POINTS, HOP, k.TO)
        feed.squelch = ssl.SlotSquelch(src, fcw, np.ones(sources), np.ones(sources), HALF, 0, 0)
    feed.floor = sf.Floor(sources, HALF, RO, RC, rise, fall, fmin)
    return feed


class Block:
    """One block of the host form, whichever mode: Y, P, state, J, floor [4][S], opens bool [C] (slot mode: any tile), and the mode's own tuple for its fetch."""

    def __init__(self, mode, e):
        self.mode, self.raw, self.floor = mode, e[:-1], e[-1]
        self.Y, self.P = e[0], e[1]
        if mode == "block":
            self.state, self.J = e[2], e[4]
            self.opens = self.all_open = (e[2] & OPEN) != 0
        else:
            state, bands, op, mask, tiles, J = e[3]
            self.state, self.J = state, J
            flags = ssl.unpack(mask, tiles)
            self.opens, self.all_open = flags.any(axis=1), flags.all(axis=1)


def _check(ctx, blk, what, back=0):
    """The fetched decisions and floor plane of a block against its host form."""
    if blk.mode == "block":
        g9._check_fetch(ctx, blk.raw, what, back)
    else:
        gs._check_fetch(ctx, blk.raw, what, back)
    plane, frames = ctx.wide_squelch_floor_fetch(back)
    assert frames == blk.J and plane.shape == blk.floor.shape, (what, frames, blk.J, plane.shape)
    _assert_words(plane, blk.floor, (what, "floor plane"))
    nan = np.isnan(blk.floor[0])
    assert (_u32(plane[0])[nan] == NAN).all(), (what, "the median of a row of NaNs is the quiet NaN")


@functools.lru_cache(maxsize=None)
def _expected(kind, mode, fmin):
    """The host form of the whole feed, and the plan asserted on it before anything runs on the device."""
    k = KINDS[kind]
    data = _source(kind)
    feed = _feed(kind, mode, data, fmin)
    out = [Block(mode, feed.block(b * k.Wb, (b + 1) * k.Wb)) for b in range(NBLOCKS)]
    opens = np.array([o.opens for o in out]).T.astype(int).tolist()
    every = np.array([o.all_open for o in out]).T.astype(int).tolist()
    zeros = [1, 1, 1, 1] if fmin == 0.0 else [0, 0, 0, 0]
    # carriers open throughout; channel 2 with its carrier and in the loud block; the empty bin of source 0 only in the loud block, where the floor has
    # risen by an eighth of the way; the zeros' channels open at levels +0 and closed at floor_min; source 2's empty bin only under the NaN bands
    assert opens == [[1, 1, 1, 1], [1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 0], zeros, zeros, [1, 1, 1, 1], [0, 0, 1, 0]], (kind, mode, fmin, opens)
    assert every[:6] == opens[:6] and every[6] == [1, 1, 1, 1], (kind, mode, every)
    F = np.array([o.floor[1] for o in out])
    med = np.array([o.floor[0] for o in out])
    assert 30.0 < F[2, 0] / F[1, 0] / 0.125 < 100.0 and abs(F[2, 0] / F[1, 0] / (1.0 + 0.125 * (med[2, 0] / med[1, 0] - 1.0)) - 1.0) < 0.1   # (the slow rise)
    assert abs(F[3, 0] / F[0, 0] - 1.0) < 0.3 and F[3, 0] < 0.25 * F[2, 0]                                                               # (the fall at once)
    assert (_u32(F[:, 1]) == _u32(np.float32(fmin))).all() and (_u32(med[:, 1]) == 0).all()                                               # (the zeros)
    assert not np.isfinite(med[2, 2]) and _u32(F[2, 2]) == _u32(F[1, 2]) and np.isfinite(F[:, 2]).all()                                   # (the carry holds)
    for o in out:
        for a in (o.Y, o.P, o.state, o.floor):
            a.setflags(write=False)
    return out


def _configure(ctx, kind, mode, fmin=0.0, src=SRC, fcw=FCW, sources=3, floor=True, rise=RISE, fall=FALL, fmt=F32):
    KINDS[kind].configure(ctx, fmt, sources)
    ctx.wide_channels(src, fcw)
    ctx.reset()
    ctx.wide_spectrum(POINTS, HOP)
    _mode(ctx, mode, np.ones(sources, dtype=np.float32))
    if floor:
        ctx.wide_squelch_floor(RO, RC, rise, fall, fmin)


def _mode(ctx, mode, o, c=None):
    if mode == "block":
        ctx.wide_squelch(HALF, o, o if c is None else c, 0)
    else:
        ctx.wide_squelch_slots(HALF, o, o if c is None else c, 0, 0)


def _upload(ctx, dev, kind, b, W, channels=8, a=None, T=None):
    k = KINDS[kind]
    ctx.upload_wide_device(dev.data_ptr() + (b * k.Wb if a is None else a) * 8, channels, k.T if T is None else T, W, GAIN)


def _floor_raw(ctx, *args):
    return ctx.lib.m17hip_wide_squelch_floor(ctx.h, *[C.c_float(v) for v in args])


def _fetch_raw(ctx, back=0, cap=16, null=False):
    plane = np.full(max(cap, 1), 7.0, dtype=np.float32)
    n, frames = C.c_uint32(78), C.c_uint32(79)
    code = ctx.lib.m17hip_wide_squelch_floor_fetch(ctx.h, C.c_uint32(back), None if null else ol._p(plane), C.c_uint64(cap), C.byref(n), C.byref(frames))
    assert code == 0 or ((plane == 7.0).all() and (n.value, frames.value) == (78, 79))   # (a refusal writes nothing)
    return code


# ---- 1: four blocks under each tuner and each mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_block_is_the_host_forms(kind, mode):
    k = KINDS[kind]
    data = _source(kind)
    dev = _dev(data)
    ctx = m17hip.Context(8, k.T)
    try:
        for fmin in (0.0, 1.0):   # (the second pass: the zeros' channels closed by floor_min)
            exp = _expected(kind, mode, fmin)
            Y, P = np.concatenate([e.Y for e in exp], axis=1), np.concatenate([e.P for e in exp], axis=1)
            _configure(ctx, kind, mode, fmin)
            ctx.wide_meter(48)
            assert _fetch_raw(ctx) == ESTATE
            for b in range(NBLOCKS):
                _upload(ctx, dev, kind, b, data.shape[1])
                _assert_words(ctx.download_f32(), exp[b].Y, (kind, mode, fmin, b))
                _check(ctx, exp[b], (kind, mode, fmin, b))
                if b:
                    _check(ctx, exp[b - 1], (kind, mode, fmin, b, "back"), back=1)
                else:
                    assert _fetch_raw(ctx, 1) == ESTATE
                planes, fw, fo, t = ctx.wide_meter_fetch()
                assert (fo, t) == (b * k.T, k.T)
                _assert_words(planes, ml.planes(P, Y, b * k.T, (b + 1) * k.T, b * k.T, 48), (kind, mode, b, "meter"))
    finally:
        ctx.close()


# ---- 2: 4096 points -----------------------------------------------------------------------------------------------------------------------------------------------
BIG, BIG_T = 4096, 2458   # (12 290 samples a block: two frames at the least, whatever the block's place in the feed)


@functools.lru_cache(maxsize=None)
def _big_source():
    """int16 [4][2 x W]: source 0 has carriers in just under half its bins, source 1 in just over half, source 2 is source 0 again, source 3 a pure tone of
    period 4 with no noise (its samples are exact, and most of its bins hold equal words)."""
    W = 2 * BIG_T * 5
    rng = np.random.default_rng(6213)
    n = np.arange(W)
    x = np.zeros((4, W), dtype=np.complex128)
    for s, raised in ((0, 2036), (1, 2060)):   # (bins 0 .. raised - 1 at one magnitude, signs alternating: a pulse in the middle of every aligned frame)
        spec = np.zeros(BIG, dtype=np.complex128)
        spec[:raised] = 12.0 * (-1.0) ** np.arange(raised)
        period = np.fft.ifft(spec) * BIG
        x[s] = period[n % BIG] + 2.0 * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    x[2] = x[0]
    x[3] = 8000.0 * np.exp(2j * np.pi * n / 4.0)
    data = g9._as_format(x, wl.IQ_I16)
    data[3] = np.array([[8000, 0], [0, 8000], [-8000, 0], [0, -8000]], dtype=np.int16)[n % 4]
    data.setflags(write=False)
    return data


BIG_SRC = [0, 1, 2, 3, 0, 1, 3, 3]
BIG_FCW = [1000 << 20, 1000 << 20, 1000 << 20, 1 << 30, -(1000 << 20), -(1000 << 20), 0, 1 << 29]   # (bin 1000 raised in 0..2, bin 3096 in none; the tone's bin 1024)


@functools.lru_cache(maxsize=None)
def _big_expected():
    data = _big_source()
    W = BIG_T * 5
    src, fcw = BIG_SRC, BIG_FCW
    taps = m17hip.wide_default_taps(5)
    feed = sf.Feed([wl.Tuner(taps, 5, w, GAIN) for w in fcw], src, data, BIG, BIG)
    feed.squelch = sq.Squelch(src, fcw, np.ones(4), np.ones(4), 4, 0)
    feed.floor = sf.Floor(4, 4, RO, RC, RISE, FALL, 0.0)
    exp = [Block("block", feed.block(b * W, (b + 1) * W)) for b in range(2)]
    planes = [spl.plane(data[s][:W], BIG, BIG)[0] for s in range(4)]
    assert all(e.J >= 2 for e in exp)
    med = exp[0].floor[0]
    assert med[1] > 1000.0 * med[0] and _u32(med[0]) == _u32(med[2])            # (under half: the floor; over half: a carrier; the same samples: the same word)
    # a carrier in a source whose median is the floor opens; the same carrier in the source whose median is a carrier does not; the empty bins are closed
    assert exp[0].opens[:6].tolist() == [True, False, True, True, False, False], exp[0].opens
    keys = sf.keys_stated(planes[3])   # (ties at the rank: the median's word stands more than once in the pure tone's row)
    assert int((keys == np.sort(keys)[BIG // 2]).sum()) >= 2
    return exp


def test_4096_points_and_ties_at_the_rank():
    data = _big_source()
    W = BIG_T * 5
    src, fcw = BIG_SRC, BIG_FCW
    exp = _big_expected()
    ctx = m17hip.Context(8, BIG_T)
    try:
        ctx.wide_config(4, 5, wl.IQ_I16)
        ctx.wide_channels(src, fcw)
        ctx.reset()
        ctx.wide_spectrum(BIG, BIG)
        ctx.wide_squelch(4, np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32), 0)
        ctx.wide_squelch_floor(RO, RC, RISE, FALL, 0.0)
        dev = _dev(data)
        for b in range(2):
            ctx.upload_wide_device(dev.data_ptr() + b * W * 4, 8, BIG_T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), exp[b].Y, b)
            _check(ctx, exp[b], ("4096", b))
    finally:
        ctx.close()


# ---- 3: blocks without a frame ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_block_without_a_frame_leaves_the_floor(mode):
    """wide_config at R = 5: a block of 10 outputs is 50 samples, shorter than the 64 points.  As the first block every channel is open, the carry is still a
    NaN and so are the fetched levels; behind a whole block it has that block's carry and levels."""
    kind = "config"
    k = KINDS[kind]
    data = _source(kind)
    feed = _feed(kind, mode, data)
    cuts = [0, 50, 50 + k.Wb, 100 + k.Wb, 100 + 2 * k.Wb]
    exp = [Block(mode, feed.block(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [e.J > 0 for e in exp] == [False, True, False, True]
    assert np.isnan(exp[0].floor[1:]).all() and exp[0].opens.all() and exp[2].opens.all()
    assert np.array_equal(_u32(exp[2].floor[1:]), _u32(exp[1].floor[1:])) and np.isfinite(exp[2].floor[1:, 0]).all()
    ctx = m17hip.Context(8, k.T)
    try:
        _configure(ctx, kind, mode)
        dev = _dev(data)
        for b, T in enumerate((10, k.T, 10, k.T)):
            _upload(ctx, dev, kind, b, data.shape[1], a=cuts[b], T=T)
            _assert_words(ctx.download_f32()[:, :T], exp[b].Y, (mode, b))
            _check(ctx, exp[b], (mode, b))
    finally:
        ctx.close()


# ---- 4: ordering and what starts the floor over ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_blocks_in_flight_then_resets_and_a_retune(mode):
    """Block 0 staged on the copy stream, block 1 in place on the main stream, no wait in between, then the staged block's run: the floor carry follows the
    feed's order across the streams.  Then: m17hip_demod_reset_channels leaves the floor (block 2's rise by an eighth shows it), a retune keeps it,
    m17hip_demod_reset and m17hip_wide_squelch_floor each start it over."""
    kind = "config"
    T, Wb = 960, 4800   # (whole carrier-detect ticks of 192 outputs, so that a channel reset may follow the run)
    data = _source(kind)
    feed = _feed(kind, mode, data)
    ctx = m17hip.Context(8, T)
    try:
        _configure(ctx, kind, mode)
        dev = _dev(data)
        W = data.shape[1]
        e0, e1 = (Block(mode, feed.block(b * Wb, (b + 1) * Wb)) for b in range(2))
        ctx._upload_wide_raw("m17hip_upload_wide_device_async", dev.data_ptr(), 8, T, W, GAIN)
        _upload(ctx, dev, kind, 1, W, a=Wb, T=T)
        _check(ctx, e0, "staged", back=1)
        _check(ctx, e1, "in place", back=0)
        ctx.run(channels=8, samples=T)   # (the staged block's)
        _assert_words(ctx.download_f32(), e0.Y, "the staged block's slab")
        ctx.upload_wait()
        # a channel reset and a retune: the floor stands, so block 2's is the slow rise from block 1's
        ctx.reset_channels([3])
        feed.reset([3])
        ctx.wide_channels(SRC, FCW[:3] + [21 << 26] + FCW[4:])
        feed.tuners[3].fcw = 21 << 26
        feed.squelch.fcw[3] = 21 << 26
        e2 = Block(mode, feed.block(2 * Wb, 3 * Wb))
        assert e1.floor[1, 0] < e2.floor[1, 0] < 0.5 * e2.floor[0, 0] * 3.0 / e2.J   # (kept: started over it would be the block's own floor)
        _upload(ctx, dev, kind, 2, W, a=2 * Wb, T=T)
        _assert_words(ctx.download_f32(), e2.Y, "block 2")
        _check(ctx, e2, "block 2: the floor kept")
        # m17hip_demod_reset: the floor starts over — the loud block again, now as the first, sets the floor at once
        ctx.reset()
        assert _fetch_raw(ctx) == ESTATE
        feed.reset()
        e = Block(mode, feed.block(2 * Wb, 3 * Wb))
        assert abs(e.floor[1, 0] * e.J / e.floor[0, 0] / 3.0 - 1.0) < 1e-6 and not e.opens[3]
        _upload(ctx, dev, kind, 2, W, a=2 * Wb, T=T)
        _assert_words(ctx.download_f32(), e.Y, "after reset")
        _check(ctx, e, "after reset")
        # the call itself: the same again, with the feed's count and histories going on
        ctx.wide_squelch_floor(RO, RC, RISE, FALL, 0.0)
        assert _fetch_raw(ctx) == ESTATE
        feed.floor.reset()
        feed.squelch.reset()
        e = Block(mode, feed.block(2 * Wb, 3 * Wb))
        _upload(ctx, dev, kind, 2, W, a=2 * Wb, T=T)
        _assert_words(ctx.download_f32(), e.Y, "after the call")
        _check(ctx, e, "after the call")
    finally:
        ctx.close()


# ---- 5 and 6: equivalence with given levels, off and back ------------------------------------------------------------------------------------------------------------
def _words(ctx, mode):
    """Everything a block leaves, as uint32 arrays."""
    y = ctx.download_f32().copy().view(np.uint32)
    if mode == "block":
        o, h, band, frames = ctx.wide_squelch_fetch()
        return [y, h | (o.astype(np.uint32) << 31), band.view(np.uint32)]
    state, bands, mask, tiles, frames = ctx.wide_squelch_slots_fetch()
    return [y, state, bands.view(np.uint32), mask]


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        nan = np.isnan(v.view(np.float32)) if i in (0, 2) else np.zeros(v.shape, dtype=bool)
        assert u.shape == v.shape and np.array_equal(u[~nan], v[~nan]) and np.isnan(u.view(np.float32)[nan]).all(), (what, i)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_given_levels_equal_to_the_devices_give_the_same_words_and_off_restores_them(kind, mode):
    """Context A has the mode on.  Context B gets, per block, the levels A's fetch returned as given levels — through the squelch call, which starts the hold
    counts over, so hang is 0 here and no count is carried.  State words, bands, masks and slabs are equal: the unchanged squelch kernels read the floor plane
    as they read the table.  Sources 0 and 2 only (given levels must be finite and positive).  Then A turns the mode off: the given levels it was configured
    with serve again from the next block, and the words are those of a context C that never had it on; a squelch call turns it off as well; and C's timer
    shows that nothing was queued."""
    k = KINDS[kind]
    data = _source(kind)[[0, 2]]
    src, fcw = [0, 0, 0, 0, 1, 1], FCW[:4] + FCW[6:]
    W = data.shape[1]
    dev = _dev(data)
    given = np.array([1.0e7, 1.0e7], dtype=np.float32)   # (between the loud block's noise band and a carrier's)
    a, b, c = (m17hip.Context(6, k.T) for _ in range(3))
    try:
        _configure(a, kind, mode, src=src, fcw=fcw, sources=2, rise=1.0)
        _mode(a, mode, given)
        a.wide_squelch_floor(RO, RC, 1.0, FALL, 0.0)
        for x in (b, c):
            _configure(x, kind, mode, src=src, fcw=fcw, sources=2, floor=False)
            _mode(x, mode, given)
            x.timing(True)
            x.timing_reset()
        a.timing(True)
        a.timing_reset()
        for blk in (0, 1, 3):   # (not the block of the inf and the NaN: its floor is no level a caller may give)
            _upload(a, dev, kind, blk, W, channels=6)
            plane, frames = a.wide_squelch_floor_fetch()
            assert np.isfinite(plane).all() and (plane[3] > 0).all()
            _mode(b, mode, plane[2], plane[3])
            _upload(b, dev, kind, blk, W, channels=6)
            _same(_words(a, mode), _words(b, mode), (kind, mode, blk))
            _upload(c, dev, kind, blk, W, channels=6)
        assert a.timing_get("squelch_floor")[1] == 3 and a.timing_get("squelch_floor")[0] > 0.0
        assert c.timing_get("squelch_floor")[1] == 0 and b.timing_get("squelch_floor")[1] == 0
        assert c.timing_get("squelch" if mode == "block" else "squelch_slots")[1] == 3
        # off: A's given levels serve again; C has had them all along (hang 0: no count is carried into the block)
        a.wide_squelch_floor(0.0, 0.0)
        assert _fetch_raw(a) == ESTATE
        _upload(a, dev, kind, 2, W, channels=6)
        _upload(c, dev, kind, 2, W, channels=6)
        _same(_words(a, mode), _words(c, mode), (kind, mode, "off"))
        assert a.timing_get("squelch_floor")[1] == 3
        # on again, then off by a squelch call
        a.wide_squelch_floor(RO, RC)
        _upload(a, dev, kind, 3, W, channels=6)
        _upload(c, dev, kind, 3, W, channels=6)   # (C's feed goes along)
        assert _fetch_raw(a) == 0
        _mode(a, mode, given)
        assert _fetch_raw(a) == ESTATE
        _upload(a, dev, kind, 3, W, channels=6)
        _upload(c, dev, kind, 3, W, channels=6)
        _same(_words(a, mode), _words(c, mode), (kind, mode, "off by the squelch call"))
        assert a.timing_get("squelch_floor")[1] == 4
    finally:
        for x in (a, b, c):
            x.close()


# ---- 7: limits and errors on a live context ----------------------------------------------------------------------------------------------------------------------------
def test_256_sources():
    """256 int16 sources of 640 samples each (ten frames), a channel on each of a few: every source's row of the floor plane is the host form's."""
    S, T = 256, 128
    rng = np.random.default_rng(6214)
    W = T * 5
    scale = 10.0 ** rng.uniform(0.0, 3.0, (S, 1))
    x = scale * (rng.standard_normal((S, W)) + 1j * rng.standard_normal((S, W)))
    x[7] = 0.0
    data = g9._as_format(x, wl.IQ_I16)
    src, fcw = [0, 7, 128, 255], [10 << 26] * 4
    floor = sf.Floor(S, HALF, RO, RC)
    got = [spl.plane(data[s], POINTS, HOP) for s in range(S)]
    plane, J = np.stack([g[0] for g in got]), got[0][1]
    exp = floor.block(plane, J)
    dec = sq.Squelch(src, fcw, exp[2], exp[3], HALF, 0)
    state, band = dec.block(plane, J)
    ctx = m17hip.Context(4, T)
    try:
        ctx.wide_config(S, 5, wl.IQ_I16)
        ctx.wide_channels(src, fcw)
        ctx.reset()
        ctx.wide_spectrum(POINTS, HOP)
        ctx.wide_squelch(HALF, np.ones(S, dtype=np.float32), np.ones(S, dtype=np.float32), 0)
        before = ctx.iq_bytes()
        ctx.wide_squelch_floor(RO, RC)
        dev = _dev(data)
        ctx.upload_wide_device(dev.data_ptr(), 4, T, W, GAIN)
        got, frames = ctx.wide_squelch_floor_fetch()
        assert frames == J == 10 and got.shape == (4, S)
        _assert_words(got, exp, "256 sources")
        o, h, b, _ = ctx.wide_squelch_fetch()
        assert np.array_equal(h | (o.astype(np.uint32) << 31), state)
        _assert_words(b, band, "bands")
        assert ctx.iq_bytes() >= before + (256 + 2 * 4 * 256) * 4
        assert _fetch_raw(ctx, 0, cap=4 * S - 1) == EINVAL and _fetch_raw(ctx, 0, cap=4 * S) == 0
    finally:
        ctx.close()


def test_state_and_argument_errors_on_a_live_context():
    kind = "config"
    k = KINDS[kind]
    data = _source(kind)
    inf, nan = float("inf"), float("nan")
    ok = (float(RO), float(RC), 0.125, 1.0, 0.0)
    ctx = m17hip.Context(8, k.T)
    try:
        assert _floor_raw(ctx, *ok) == ESTATE and _floor_raw(ctx, 0.0, 0.0, 1.0, 1.0, 0.0) == ESTATE   # (no wideband configuration)
        k.configure(ctx, F32)
        ctx.wide_channels(SRC, FCW)
        ctx.reset()
        ctx.wide_spectrum(POINTS, HOP)
        assert _floor_raw(ctx, *ok) == ESTATE            # (no squelch mode on)
        assert _floor_raw(ctx, 0.0, 0.0, 1.0, 1.0, 0.0) == 0   # (off is off)
        assert _fetch_raw(ctx) == ESTATE
        ones = np.ones(3, dtype=np.float32)
        dev = _dev(data)
        for mode in MODES:
            _mode(ctx, mode, ones)
            for bad in ((nan,) + ok[1:], (ok[0], inf) + ok[2:], ok[:2] + (nan, 1.0, 0.0), ok[:3] + (-inf, 0.0), ok[:4] + (inf,),
                        (float(RC), float(RO)) + ok[2:], (ok[0], 0.0) + ok[2:], (ok[0], -1.0) + ok[2:], (0.0, -0.5) + ok[2:], (-2.0, -3.0) + ok[2:],
                        ok[:2] + (0.0, 1.0, 0.0), ok[:2] + (1.5, 1.0, 0.0), ok[:2] + (1.0, 0.0, 0.0), ok[:2] + (1.0, 1.0000001, 0.0),
                        ok[:2] + (-0.5, 1.0, 0.0), ok[:4] + (-1.0e-30,), (0.0, 0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0, -1.0)):
                assert _floor_raw(ctx, *bad) == EINVAL, bad
            assert _floor_raw(ctx, *ok) == 0 and _floor_raw(ctx, 5.0, 5.0, 1.0, 1.0e-6, 1.0e30) == 0 and _floor_raw(ctx, *ok) == 0
            assert _fetch_raw(ctx) == ESTATE and _fetch_raw(ctx, 2) == EINVAL
            _upload(ctx, dev, kind, 0, data.shape[1])
            assert _fetch_raw(ctx) == 0 and _fetch_raw(ctx, 1) == ESTATE and _fetch_raw(ctx, 2) == EINVAL
            assert _fetch_raw(ctx, 0, cap=11) == EINVAL and _fetch_raw(ctx, 0, cap=12) == 0 and _fetch_raw(ctx, 0, null=True) == EINVAL
            assert ctx.lib.m17hip_wide_squelch_floor_fetch(ctx.h, C.c_uint32(0), ol._p(np.zeros(12, dtype=np.float32)), C.c_uint64(12), None, None) == 0
            first, _ = ctx.wide_squelch_floor_fetch()
            _upload(ctx, dev, kind, 1, data.shape[1])
            back, _ = ctx.wide_squelch_floor_fetch(1)
            assert np.array_equal(_u32(back), _u32(first)) and not np.array_equal(_u32(ctx.wide_squelch_floor_fetch(0)[0]), _u32(first))
        # between m17hip_demod_front and its run
        ctx._upload_wide_raw("m17hip_upload_wide_device_async", dev.data_ptr(), 8, k.T, data.shape[1], GAIN)
        ctx.front(channels=8, samples=k.T)
        assert _floor_raw(ctx, *ok) == ESTATE and _floor_raw(ctx, 0.0, 0.0, 1.0, 1.0, 0.0) == ESTATE
        ctx.run(channels=8, samples=k.T)
        assert _floor_raw(ctx, *ok) == 0
        # everything that turns the squelch off turns it off
        ctx.wide_spectrum(POINTS, HOP)
        assert _fetch_raw(ctx) == ESTATE and _floor_raw(ctx, *ok) == ESTATE
        # under the raster no squelch mode can be on
        ctx.wide_raster(2, 5, 48)
        ctx.wide_spectrum(POINTS, HOP)
        assert _floor_raw(ctx, *ok) == ESTATE and _floor_raw(ctx, 0.0, 0.0, 1.0, 1.0, 0.0) == 0
    finally:
        ctx.close()


# ---- 8: the example ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", (False, True))
def test_the_example_with_the_floor_on_the_device(slots):
    """examples/m17-demod-gpu --spectrum 2048 --squelch 10 --auto-floor [--slots] on tests/test_wide_squelch_slots.py's source with 20 ms of noise in front
    (the first block is squelched too, and the demodulator does not survive a long run of exact zeros from its very first sample: NOTES.md): it prints
    the frames the unsquelched run decodes (those of a Viterbi cost under 30, as the CPU tests count them) and a floor per block, the first block included."""
    import test_wide_squelch_slots as cpu
    bb, row = cpu._late_transmission(320 * 128)
    exe = os.path.join(wl.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    raw = np.ascontiguousarray(row).tobytes()

    def run(*more):
        r = subprocess.run([exe, "--wide-i16", "--rate", "2048000", "--offset-hz", "12500", "--spectrum", "2048", *more], input=raw, capture_output=True,
                           check=True, timeout=120)
        err = r.stderr.decode().split("\n")
        return [l for l in r.stdout.decode().split("\n") if l.strip()], [float(m.group(1)) for m in (re.match(r"floor: (-?[0-9.]+) dB", l) for l in err) if m]

    plain, none = run()
    kept, floors = run("--squelch", "10", "--auto-floor", *(["--slots", "--lead", "1", "--hang", "1"] if slots else ["--hang", "1"]))
    good = lambda lines: [l for l in lines if int(l.split()[1]) < 30]   # (type, Viterbi cost, payload: the unsquelched run also "decodes" the noise behind the transmission, at costs over 100)
    assert len(good(plain)) >= 6 and good(kept) == good(plain) and not none
    blocks = -(-(row.shape[0] // 128 * 3) // 1920)
    assert len(floors) >= blocks - 1 and max(floors) - min(floors) < 10.0, floors
