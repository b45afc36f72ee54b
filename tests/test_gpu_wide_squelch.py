"""GPU tests of the spectrum squelch (ABI 619, include/m17hip.h: m17hip_wide_squelch): wide_squelch_kernel decides per block and channel from the block's own
spectrum, and the squelched instantiations of tune_kernel, tune2_kernel and resample_kernel store zeros for a closed channel and return.  Every comparison
is exact: the downloaded float slab, the fetched state words and band powers and the meter's planes as uint32 words against the HOST form (tests/squelch_lib.py:
detail/core.h under the host compiler over spectrum_lib's planes and the three tuners' host forms).  What the host form itself is worth is asserted without a
GPU in tests/test_wide_squelch.py.

The shapes are the smallest that can go wrong: 2 sources, 6 channels — two share a source and a word, one sits on each source's edge word, one never hears
anything —, 64 points at hop 64, blocks of two tiles per channel (300 outputs under the integer tuners, 900 under the resampler, whose tile is 255 groups of
3), so the tile boundary and the tile that holds output T - 1 are different workgroups.  The sources are tones switched per block over low noise."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import meter_lib as ml
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_lib as sq
import test_gpu_wide_input as g1
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
OPEN = sq.OPEN
FMTS, SB = g1.FMTS, g1.SB
_u32, _assert_words, _dev = g1._u32, g1._assert_words, g1._dev
GAIN = 5.0 / 3.0
POINTS, HOP, HALF = 64, 64, 1
OPEN_DB, CLOSE_DB = 20.0, 10.0
NBLOCKS = 6

# the channels: (source, frequency word).  0 and 1 share source 0 and a word (bin 10); 2 and 3 sit on the edge words of source 0 and 1 (both bin 32);
# 4 listens between two bins' centres (bin 51 of source 1); 5 to bin 20 of source 1, where nothing ever is
SRC = [0, 0, 0, 1, 1, 1]
FCW = [10 << 26, 10 << 26, -(1 << 31), (1 << 31) - 1, -(13 << 26) + 12345678, 20 << 26]
# the tones: (source, word, amplitude per block in units of the format's strong tone; W = the weak one, between the close and the open level)
W_ = -1.0
TONES = [(0, FCW[0], (1, W_, 0, W_, 1, 0)), (0, FCW[2], (0, 1, 1, 0, 0, 1)), (1, FCW[3], (1, 0, 0, 1, 1, 0)), (1, FCW[4], (0, 0, 1, 0, 0, 1))]
# what the schedule is made for, per channel and block (asserted on the host form before anything runs on the device)
PLAN = {0: [[1, 1, 0, 0, 1, 0], [1, 1, 0, 0, 1, 0], [0, 1, 1, 0, 0, 1], [1, 0, 0, 1, 1, 0], [0, 0, 1, 0, 0, 1], [0] * 6],
        2: [[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0] * 6]}
AMPL = {wl.IQ_I16: (5000.0, 33.0, 20.0), wl.IQ_F32: (5000.0, 33.0, 20.0), wl.IQ_U8: (100.0, 3.3, 2.0)}   # strong, weak, noise sigma per component


class Kind:
    """One of the three tuners: T outputs per block, g source samples per u outputs, configure(ctx, fmt) and tuner(fcw) -> its host form."""


def _kinds():
    out = {}
    k = Kind()
    k.T, k.u, k.g = 300, 1, 5
    taps = m17hip.wide_default_taps(5)
    k.configure = lambda ctx, fmt: ctx.wide_config(2, 5, fmt)
    k.tuner = lambda w: wl.Tuner(taps, 5, w, GAIN)
    k.timer = "tune"
    out["config"] = k
    k = Kind()
    k.T, k.u, k.g = 300, 1, 6
    t1, t2 = m17hip.wide_default_taps2(2, 3)
    k.configure = lambda ctx, fmt: ctx.wide_config2(2, 2, 3, fmt)
    k.tuner = lambda w: w2.Tuner2(t1, 2, t2, 3, w, GAIN)
    k.timer = "tune2"
    out["config2"] = k
    k = Kind()
    k.T, k.u, k.g = 900, 3, 8 * 16
    r1, r2 = m17hip.wide_resample_default_taps(16, 3, 8)
    k.configure = lambda ctx, fmt: ctx.wide_resample(2, 16, 3, 8, fmt)
    k.tuner = lambda w: rl.Resampler(r1, 16, 3, 8, r2, w, GAIN)
    k.timer = "resample"
    out["resample"] = k
    return out


KINDS = _kinds()


def _as_format(x, fmt):
    """complex128 [S][W] in the format's units -> the format's array."""
    if fmt == wl.IQ_F32:
        return x.astype(np.complex64)
    iq = np.stack([x.real, x.imag], axis=-1)
    if fmt == wl.IQ_I16:
        return np.clip(np.rint(iq), -32768, 32767).astype(np.int16)
    return np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _source(kind, fmt, nblocks=NBLOCKS):
    """(data [2][nblocks x W] of the format, read-only; the levels (open[2], close[2]) from the host-form plane of a block of the same noise alone)."""
    k = KINDS[kind]
    Wb = k.T // k.u * k.g
    strong, weak, sigma = AMPL[fmt]
    rng = np.random.default_rng(6190 + len(kind) + 7 * fmt)
    n = np.arange(nblocks * Wb)
    x = sigma * (rng.standard_normal((2, n.size)) + 1j * rng.standard_normal((2, n.size)))
    for s, word, ampl in TONES:
        a = np.repeat([strong if v == 1 else weak if v == W_ else 0.0 for v in ampl[:nblocks]], Wb)
        x[s] += a * np.exp(2j * np.pi * ((word * n) % (1 << 32)) / float(1 << 32))
    data = _as_format(x, fmt)
    noise = _as_format(sigma * (rng.standard_normal((2, Wb)) + 1j * rng.standard_normal((2, Wb))), fmt)
    got = [spl.plane(noise[s], POINTS, HOP) for s in range(2)]
    levels = m17hip.wide_squelch_levels(np.stack([g[0] for g in got]), got[0][1], HALF, OPEN_DB, CLOSE_DB)
    data.setflags(write=False)
    return data, levels


def _feed(kind, data, levels, hang, squelched=True):
    k = KINDS[kind]
    feed = sq.Feed([k.tuner(w) for w in FCW], SRC, data, POINTS, HOP)
    if squelched:
        feed.squelch = sq.Squelch(SRC, FCW, levels[0], levels[1], HALF, hang)
    return feed


@functools.lru_cache(maxsize=None)
def _expected(kind, fmt, hang):
    """The host form of the whole feed of _source: per block (Y, P, state, band, J), read-only; the plan is what it shows."""
    k = KINDS[kind]
    data, levels = _source(kind, fmt)
    Wb = k.T // k.u * k.g
    feed = _feed(kind, data, levels, hang)
    out = [feed.block(b * Wb, (b + 1) * Wb) for b in range(NBLOCKS)]
    opens = np.array([(o[2] & OPEN) != 0 for o in out]).T.astype(int)
    assert opens.tolist() == PLAN[hang], (kind, fmt, hang, opens.tolist(), [o[3].tolist() for o in out], levels)
    if hang == 0:   # (the first output after the reopening of channel 0 in block 4 is +0, the rest of the block is not)
        assert _u32(out[4][0][0, :1]) == 0 and (out[4][0][0, 1:] != 0).any() and (_u32(out[2][0][0]) == 0).all()
    for o in out:
        for a in o[:4]:
            a.setflags(write=False)
    return out


def _squelch(ctx, levels, hang, half=HALF):
    ctx.wide_squelch(half, levels[0], levels[1], hang)


def _fetch_raw(ctx, back=0, cap=8):
    state, band = np.full(cap, 77, dtype=np.uint32), np.full(cap, 7.0, dtype=np.float32)
    n, frames = C.c_uint32(78), C.c_uint32(79)
    code = ctx.lib.m17hip_wide_squelch_fetch(ctx.h, C.c_uint32(back), ol._p(state), ol._p(band), C.c_uint64(cap), C.byref(n), C.byref(frames))
    assert code == 0 or ((state == 77).all() and (band == 7.0).all() and (n.value, frames.value) == (78, 79))   # (a refusal writes nothing)
    return code


def _check_fetch(ctx, exp, what, back=0):
    Y, P, state, band, J = exp
    o, h, b, frames = ctx.wide_squelch_fetch(back)
    assert o.size == state.size and frames == J, (what, o.size, frames, J)
    assert np.array_equal(o, (state & OPEN) != 0) and np.array_equal(h, state & ~np.uint32(OPEN)), (what, o, h, state)
    _assert_words(b, band, (what, "band"))


def _configure(ctx, kind, fmt):
    KINDS[kind].configure(ctx, fmt)
    ctx.wide_channels(SRC, FCW)
    ctx.reset()
    ctx.wide_spectrum(POINTS, HOP)


class Uploader:
    """One of the four entry points over the blocks of one feed: block(k) uploads block k (and runs it where it was staged), so that download_f32 has it."""

    def __init__(self, ctx, kind, fmt, data, name):
        import torch
        self.ctx, self.k, self.fmt, self.name = ctx, KINDS[kind], fmt, name
        self.Wb = self.k.T // self.k.u * self.k.g
        self.host = np.array(data)
        self.W = self.host.shape[1]
        self.dev = _dev(data) if "device" in name else None
        self.pin = torch.from_numpy(self.host).pin_memory() if name == "m17hip_upload_wide_async" else None

    def block(self, b, channels=6, samples=None, run=True):
        T = self.k.T if samples is None else samples
        off = b * self.Wb * SB[self.fmt]
        base = self.dev.data_ptr() if self.dev is not None else self.pin.data_ptr() if self.pin is not None else self.host.ctypes.data
        self.ctx._upload_wide_raw(self.name, base + off, channels, T, self.W, GAIN)
        if self.name.endswith("_async") and run:
            self.ctx.run(channels=channels, samples=T)


NAMES = ("m17hip_upload_wide", "m17hip_upload_wide_async", "m17hip_upload_wide_device", "m17hip_upload_wide_device_async")


# ---- 1: the three tuners, the three formats, the four ways in -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", ("i16", "f32", "u8"))
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_block_is_the_host_forms(kind, fmt, name):
    """Six blocks in which channels open, hold on a weak tone, close, stay closed on the same weak tone and reopen (hang 0): the float slab, the state words
    and the band powers of every block, and the block before's through back = 1."""
    f = FMTS[fmt]
    data, levels = _source(kind, f)
    exp = _expected(kind, f, 0)
    ctx = m17hip.Context(6, KINDS[kind].T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 0)
        up = Uploader(ctx, kind, f, data, name)
        for b in range(NBLOCKS):
            up.block(b)
            _assert_words(ctx.download_f32(), exp[b][0], (kind, fmt, name, b))
            _check_fetch(ctx, exp[b], (kind, fmt, name, b))
            if b:
                _check_fetch(ctx, exp[b - 1], (kind, fmt, name, b, "back"), back=1)
            else:
                assert _fetch_raw(ctx, 1) == ESTATE
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_hang_2_and_the_meter_on(kind):
    """The same feed at hang 2 with the meter on at window 48: the meter's planes are meter_lib's over the squelched z and y — zeros where closed —, and the
    spectrum's fetch is what it was."""
    f = wl.IQ_I16
    data, levels = _source(kind, f)
    exp = _expected(kind, f, 2)
    T = KINDS[kind].T
    Y, P = np.concatenate([e[0] for e in exp], axis=1), np.concatenate([e[1] for e in exp], axis=1)
    ctx = m17hip.Context(6, T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 2)
        ctx.wide_meter(48)
        up = Uploader(ctx, kind, f, data, NAMES[2])
        for b in range(NBLOCKS):
            up.block(b)
            _assert_words(ctx.download_f32(), exp[b][0], (kind, b))
            _check_fetch(ctx, exp[b], (kind, b))
            planes, fw, fo, t = ctx.wide_meter_fetch()
            assert (fo, t) == (b * T, T)
            _assert_words(planes, ml.planes(P, Y, b * T, (b + 1) * T, b * T, 48), (kind, b, "meter"))
            power, frames, first = ctx.wide_spectrum_fetch()
            Wb = up.Wb
            ref = spl.planes(data, POINTS, HOP, [b * Wb, (b + 1) * Wb])[0]
            assert frames == ref[1] == exp[b][4] and first == ref[2]
            _assert_words(power, ref[0], (kind, b, "spectrum"))
    finally:
        ctx.close()


# ---- 2: all open, all closed, no frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_all_open_is_the_unsquelched_feed_and_all_closed_is_all_zero(kind):
    f = wl.IQ_I16
    data, levels = _source(kind, f)
    k = KINDS[kind]
    plain = _feed(kind, data, levels, 0, squelched=False)
    ref = [plain.block(b * (k.T // k.u * k.g), (b + 1) * (k.T // k.u * k.g))[0] for b in range(3)]
    tiny, huge = np.full(2, 1.0e-30, dtype=np.float32), np.full(2, 1.0e30, dtype=np.float32)
    ctx = m17hip.Context(6, k.T)
    try:
        got = {}
        for mode in ("off", "open", "closed"):
            _configure(ctx, kind, f)
            if mode != "off":
                _squelch(ctx, (tiny, tiny) if mode == "open" else (huge, huge), 0)
            up = Uploader(ctx, kind, f, data, NAMES[2])
            got[mode] = []
            for b in range(3):
                up.block(b)
                got[mode].append(ctx.download_f32().copy())
                if mode != "off":
                    o, h, band, frames = ctx.wide_squelch_fetch()
                    assert o.all() == (mode == "open") and o.any() == (mode == "open") and (h == (1 if mode == "open" else 0)).all() and frames > 0
        for b in range(3):
            _assert_words(got["off"][b], ref[b], (kind, b, "the host form"))
            assert np.array_equal(_u32(got["open"][b]), _u32(got["off"][b])), (kind, b)
            assert (_u32(got["closed"][b]) == 0).all(), (kind, b)
    finally:
        ctx.close()


def test_a_block_without_a_frame_is_open_and_leaves_the_holds():
    """wide_config at R = 5: a block of 10 outputs is 50 samples, shorter than the 64 points.  Between two whole blocks it is open for every channel, the
    hold counts stand, and the block behind it finds them (hang 1: channel 0, open in block 0 and silent from then on, counts 2, 2, 1)."""
    f = wl.IQ_I16
    kind = "config"
    strong, weak, sigma = AMPL[f]
    rng = np.random.default_rng(6195)
    lens = (300, 10, 300, 300)
    cuts = np.concatenate([[0], np.cumsum(lens)]) * 5
    n = np.arange(cuts[-1])
    x = sigma * (rng.standard_normal((2, n.size)) + 1j * rng.standard_normal((2, n.size)))
    x[0, : cuts[1]] += strong * np.exp(2j * np.pi * ((FCW[0] * n[: cuts[1]]) % (1 << 32)) / float(1 << 32))
    data = _as_format(x, f)
    levels = _source(kind, f)[1]
    feed = _feed(kind, data, levels, 1)
    exp = [feed.block(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [e[4] > 0 for e in exp] == [True, False, True, True]
    assert [int(e[2][0]) for e in exp] == [2 | OPEN, 2 | OPEN, 1 | OPEN, 0] and all(int(e[2][5]) == (OPEN if e[4] == 0 else 0) for e in exp)
    ctx = m17hip.Context(6, 300)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 1)
        dev = _dev(data)
        for b, T in enumerate(lens):
            ctx.upload_wide_device(dev.data_ptr() + int(cuts[b]) * 4, 6, T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), exp[b][0], b)
            _check_fetch(ctx, exp[b], b)
    finally:
        ctx.close()


# ---- 3: resets, a retune, the squelch turned off ------------------------------------------------------------------------------------------------------------------
def test_resets_clear_the_hold_a_retune_keeps_it_and_off_is_unsquelched():
    """Hang 2 under the one-stage tuner.  Behind block 1 the holds are (3, 3, 3, 2, 0, 0).  m17hip_demod_reset_channels([0, 3]) clears those two (and their
    carries); a retune of channel 1 to the empty bin keeps its count, so it is tuned there for two more blocks; m17hip_wide_squelch(off) makes the next block
    the unsquelched one from the carries as they stand (zero where the channel was closed); m17hip_demod_reset clears every count."""
    f, kind = wl.IQ_I16, "config"
    data, levels = _source(kind, f)
    Wb = 1500
    feed = _feed(kind, data, levels, 2)
    ctx = m17hip.Context(6, 300)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 2)
        up = Uploader(ctx, kind, f, data, NAMES[2])

        def both(b, what):
            e = feed.block(b * Wb, (b + 1) * Wb)
            up.block(b)
            _assert_words(ctx.download_f32(), e[0], what)
            if e[2] is not None:
                _check_fetch(ctx, e, what)
            return e

        both(0, "block 0")
        e = both(1, "block 1")
        assert (e[2] & ~np.uint32(OPEN)).tolist() == [3, 3, 3, 2, 0, 0]
        ctx.reset_channels([0, 3])
        feed.reset([0, 3])
        ctx.wide_channels([0, 0], [FCW[0], FCW[5]])   # (channel 1 to the empty bin of source 0)
        feed.tuners[1].fcw = FCW[5]
        feed.squelch.fcw[1] = FCW[5]
        e = both(2, "block 2: two counts cleared, one channel retuned")
        assert (e[2] & ~np.uint32(OPEN)).tolist() == [0, 2, 3, 0, 3, 0] and (e[0][1] != 0).any()
        e = both(3, "block 3")
        assert (e[2] & ~np.uint32(OPEN)).tolist()[1] == 1
        ctx.wide_squelch(0, None)
        feed.squelch = None
        assert _fetch_raw(ctx) == ESTATE
        e = both(4, "block 4: off")
        # (channels 0 and 5 were closed in block 3: their first outputs stand against a zero carry)
        assert (e[0] != 0).any(axis=1).all() and _u32(e[0][0, :1]) == 0 and _u32(e[0][5, :1]) == 0 and _u32(e[0][2, :1]) != 0
        # on again: the counts start at 0 whatever they were; then a reset of the feed does the same
        _squelch(ctx, levels, 2)
        feed.squelch = sq.Squelch(SRC, [FCW[0], FCW[5]] + FCW[2:], levels[0], levels[1], HALF, 2)
        e = both(5, "block 5: on again")
        assert (e[2] & ~np.uint32(OPEN)).tolist() == [0, 0, 3, 0, 3, 0]
        ctx.reset()
        assert _fetch_raw(ctx) == ESTATE
        fresh = _feed(kind, data[:, 5 * Wb:], levels, 2)
        fresh.tuners[1].fcw = FCW[5]
        fresh.squelch.fcw[1] = FCW[5]
        e = fresh.block(0, Wb)
        up.block(5)
        _assert_words(ctx.download_f32(), e[0], "after reset")
        _check_fetch(ctx, e, "after reset")
    finally:
        ctx.close()


@pytest.mark.parametrize("how", ("wide_squelch", "reset"))
def test_a_first_block_of_fewer_channels_leaves_no_stale_count_for_a_full_one(how):
    """Hang 2: two full blocks leave the counts (3, 3, 3, 2, 0, 0).  Then m17hip_wide_squelch again, or m17hip_demod_reset: EVERY count is 0, also those of
    the channels that the next block — two channels only — does not carry.  The full block behind it finds channel 2 silent: closed from a count of 0, open
    from a stale 3."""
    f, kind = wl.IQ_I16, "config"
    data, levels = _source(kind, f)
    Wb = 1500
    feed = _feed(kind, data, levels, 2)
    ctx = m17hip.Context(6, 300)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 2)
        up = Uploader(ctx, kind, f, data, NAMES[2])
        for b in range(2):
            e = feed.block(b * Wb, (b + 1) * Wb)
            up.block(b)
            _check_fetch(ctx, e, b)
        assert (e[2] & ~np.uint32(OPEN)).tolist() == [3, 3, 3, 2, 0, 0]
        if how == "reset":
            ctx.reset()
            feed = _feed(kind, data[:, 2 * Wb:], levels, 2)
            base = 2
        else:
            _squelch(ctx, levels, 2)
            feed.squelch = sq.Squelch(SRC, FCW, levels[0], levels[1], HALF, 2)
            base = 0
        e = feed.block((2 - base) * Wb, (3 - base) * Wb, channels=2)
        up.block(2, channels=2)
        _assert_words(ctx.download_f32(), e[0], (how, "two channels"))
        _check_fetch(ctx, e, (how, "two channels"))
        e = feed.block((3 - base) * Wb, (4 - base) * Wb)
        up.block(3)
        assert int(e[2][2]) == 0 and (_u32(e[0][2]) == 0).all()   # (channel 2: no tone in this block, and no count left from before)
        _assert_words(ctx.download_f32(), e[0], (how, "all six"))
        _check_fetch(ctx, e, (how, "all six"))
    finally:
        ctx.close()


# ---- 4: state ---------------------------------------------------------------------------------------------------------------------------------------------------
def _squelch_raw(ctx, half, o, c, n, hang):
    o = None if o is None else np.ascontiguousarray(o, dtype=np.float32)
    c = None if c is None else np.ascontiguousarray(c, dtype=np.float32)
    return ctx.lib.m17hip_wide_squelch(ctx.h, C.c_uint32(half), None if o is None else ol._p(o), None if c is None else ol._p(c), C.c_uint32(n), C.c_uint32(hang))


def test_state_and_limits():
    f, kind = wl.IQ_I16, "config"
    data, levels = _source(kind, f)
    exp = _expected(kind, f, 0)
    o, c = levels
    ctx = m17hip.Context(6, 300)
    try:
        assert _squelch_raw(ctx, 1, o, c, 2, 0) == ESTATE and _squelch_raw(ctx, 0, None, None, 0, 0) == ESTATE   # (no wideband configuration yet)
        KINDS[kind].configure(ctx, f)
        ctx.wide_channels(SRC, FCW)
        ctx.reset()
        assert _squelch_raw(ctx, 1, o, c, 2, 0) == ESTATE   # (the spectrum is off)
        assert _squelch_raw(ctx, 0, None, None, 0, 0) == 0   # (off is off)
        ctx.wide_spectrum(POINTS, HOP)
        for bad in ((65, o, c, 2, 0), (32, o, c, 2, 0), (1, o, c, 2, 65536), (1, o, c, 1, 0), (1, o, c, 3, 0), (1, o, None, 2, 0), (1, None, c, 2, 0),
                    (1, None, None, 2, 0), (1, o, c, 0, 0), (1, c, o, 2, 0), (1, [np.inf, 1.0], c, 2, 0), (1, o, [0.0, 1.0], 2, 0), (1, o, [-1.0, 1.0], 2, 0),
                    (1, [np.nan, 1.0], [np.nan, 1.0], 2, 0)):
            assert _squelch_raw(ctx, *bad) == EINVAL, bad
        assert _squelch_raw(ctx, 31, o, c, 2, 65535) == 0 and _squelch_raw(ctx, 0, o, o, 2, 0) == 0
        up = Uploader(ctx, kind, f, data, NAMES[2])
        up.block(0)   # (the refused calls changed nothing; the last accepted one holds: half_bins 0)
        assert _fetch_raw(ctx) == 0 and _fetch_raw(ctx, 1) == ESTATE and _fetch_raw(ctx, 2) == EINVAL and _fetch_raw(ctx, 0, cap=5) == EINVAL
        assert ctx.lib.m17hip_wide_squelch_fetch(ctx.h, C.c_uint32(0), None, None, C.c_uint64(8), None, None) == EINVAL
        # m17hip_wide_spectrum again turns it off, and so does every configuration call
        ctx.wide_spectrum(POINTS, HOP)
        assert _fetch_raw(ctx) == ESTATE
        ctx.reset()
        up.block(0)
        _assert_words(ctx.download_f32(), _feed(kind, data, levels, 0, squelched=False).block(0, up.Wb)[0], "off after wide_spectrum")
        for conf in (lambda: ctx.wide_config(2, 5), lambda: ctx.wide_config2(2, 2, 3), lambda: ctx.wide_resample(2, 16, 3, 8), lambda: ctx.wide_raster(2, 5, 48)):
            _configure(ctx, kind, f)
            _squelch(ctx, levels, 0)
            up.block(0)
            assert _fetch_raw(ctx) == 0
            conf()
            assert _fetch_raw(ctx) == ESTATE
        # under a raster there is nothing per channel to save
        ctx.wide_spectrum(POINTS, HOP)
        assert _squelch_raw(ctx, 1, o, c, 2, 0) == ESTATE and _squelch_raw(ctx, 0, None, None, 0, 0) == 0
        # between m17hip_demod_front and its run the staged block belongs to the run being made
        _configure(ctx, kind, f)
        up.block(0)
        ctx.run(channels=6, samples=300)
        staged = Uploader(ctx, kind, f, data, NAMES[3])
        staged.block(1, run=False)
        ctx.front(channels=6, samples=300)
        assert _squelch_raw(ctx, 1, o, c, 2, 0) == ESTATE and _squelch_raw(ctx, 0, None, None, 0, 0) == ESTATE
        ctx.run(channels=6, samples=300)
        ctx.upload_wait()
        assert _squelch_raw(ctx, 1, o, c, 2, 0) == 0
        # memory and timing
        _configure(ctx, kind, f)
        before = ctx.iq_bytes()
        _squelch(ctx, levels, 0)
        ctx.timing(True)
        ctx.timing_reset()
        up.block(0)
        up.block(1)
        _check_fetch(ctx, exp[1], "timed")
        ctx.download_f32()
        assert ctx.iq_bytes() >= before + 5 * 6 * 4 + 4 * 4
        ms, launches = ctx.timing_get("squelch")
        assert launches == 2 and ms > 0.0
        assert ctx.timing_get("tune")[1] == 2 and ctx.timing_get("spectrum")[1] == 2
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 5: two blocks in flight ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_staged_and_an_in_place_block_in_flight_then_a_run(kind):
    """Block 0 staged on the copy stream, block 1 in place on the main stream, no wait in between, then the staged block's run: back = 1 and back = 0 are each
    their own host form — the hold counts and the carries cross the streams behind ev_iq —, and the slab the run worked on is the staged block's."""
    f = wl.IQ_I16
    data, levels = _source(kind, f)
    exp = _expected(kind, f, 0)
    T = KINDS[kind].T
    ctx = m17hip.Context(6, T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 0)
        up = Uploader(ctx, kind, f, data, NAMES[3])
        up.block(0, run=False)
        inplace = Uploader(ctx, kind, f, data, NAMES[2])
        inplace.dev = up.dev
        inplace.block(1)
        _check_fetch(ctx, exp[0], "staged", back=1)
        _check_fetch(ctx, exp[1], "in place", back=0)
        ctx.run(channels=6, samples=T)   # (the staged block's)
        _assert_words(ctx.download_f32(), exp[0][0], "the staged block's slab")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 6: through the whole chain -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_source():
    """(x int16 [1][W][2], T): one M17 stream transmission made by the generator at 2.048 MSPS, 12.5 kHz above the centre, amplitude 6000 over noise."""
    bb = ol.generate(ol.gen_params(seed=1, kind=1, lead_in=9600, n_frames=6, tail=4800))
    T = bb.size // 1920 * 1920
    bb = bb[:T]
    tx = m17hip.Context(1, T)
    try:
        tx.upload(bb[None, :])
        tx.synth_wide_config(1, 128, 3, wl.IQ_I16, None, 300.0, 3, 0)
        tx.synth_wide_channels([0], [m17hip.wide_fcw(12500.0, 128 / 3)], 0, 6000.0)
        x = tx.synth_wide().copy()
    finally:
        tx.close()
    x.setflags(write=False)
    return x, T


def test_one_transmission_through_the_squelched_resampler_and_the_whole_chain():
    """One M17 stream transmission made by the generator at 2.048 MSPS, 12.5 kHz above the centre; the resampling tuner (16, 3 / 8) listens there and on empty
    spectrum at +400 kHz, squelched at levels from the block's own host-form plane (2048 points, a band of 9 kHz, 10 / 6 dB).  The records of the run are the
    float oracle's on the host form's floats, channel by channel: the transmission's frames, and nothing from the closed channel's zeros."""
    x, T = _chain_source()
    src, fcw = [0, 0], [m17hip.wide_fcw(12500.0, 128 / 3), m17hip.wide_fcw(400000.0, 128 / 3)]
    N = 2048
    B = m17hip.wide_squelch_half_bins(9000.0, 2048000.0, N)
    plane, J, _ = spl.plane(x[0], N, N)
    levels = m17hip.wide_squelch_levels(plane[None, :], J, B, 10.0, 6.0)
    t1, t2 = m17hip.wide_resample_default_taps(16, 3, 8)
    feed = sq.Feed([rl.Resampler(t1, 16, 3, 8, t2, w, 1.0) for w in fcw], src, x, N, N)
    feed.squelch = sq.Squelch(src, fcw, levels[0], levels[1], B, 0)
    e = feed.block(0, x.shape[1])
    assert e[0].shape == (2, T) and ((e[2] & OPEN) != 0).tolist() == [True, False]
    ctx = m17hip.Context(2, T)
    try:
        ctx.wide_resample(1, 16, 3, 8)
        ctx.wide_channels(src, fcw)
        ctx.reset()
        ctx.wide_spectrum(N, N)
        ctx.wide_squelch(B, levels[0], levels[1], 0)
        ctx.upload_wide(x, channels=2)
        ctx.run()
        recs = ctx.frames()
        _assert_words(ctx.download_f32(), e[0], "the chain's floats")
        _check_fetch(ctx, e, "the chain")
    finally:
        ctx.close()
    fields = ("seq", "sample_pos", "cost", "frame_type", "sync_type", "len", "flags", "payload")
    for c in range(2):
        want, got = fl.demod(e[0][c])[0], recs[recs["channel"] == c]
        assert len(got) == len(want), (c, len(got), len(want))
        for name in fields:
            assert np.array_equal(got[name], want[name]), (c, name)
    good = recs[(recs["channel"] == 0) & (recs["cost"] < 30) & (recs["frame_type"] != 1)]
    assert len(good) == 7 and not (recs["channel"] == 1).any()


def test_the_example_squelches_an_empty_offset_and_keeps_a_transmission():
    """examples/m17-demod-gpu --spectrum 2048 --squelch 10 on the same source, in its blocks of 1920 outputs: tuned to the transmission it prints the lines
    of the unsquelched run, every squelched block open; tuned to empty spectrum it prints no frame, every squelched block closed.  The first block runs
    unsquelched (its plane sets the levels)."""
    import os
    import subprocess
    x, T = _chain_source()
    exe = os.path.join(wl.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    raw = np.ascontiguousarray(x[0]).tobytes()

    def run(offset, *more):
        r = subprocess.run([exe, "--wide-i16", "--rate", "2048000", "--offset-hz", str(offset), "--spectrum", "2048", *more], input=raw, capture_output=True,
                           check=True, timeout=120)
        return [l for l in r.stdout.decode().split("\n") if l.strip()], [l for l in r.stderr.decode().split("\n") if l.startswith("squelch:")]

    plain, none = run(12500)
    kept, decisions = run(12500, "--squelch", "10", "--hang", "1")
    assert len(plain) >= 6 and kept == plain and not none
    assert len(decisions) == T // 1920 - 1 and all(d.startswith("squelch: open, hold 2,") for d in decisions), decisions[:3]
    silent, decisions = run(400000, "--squelch", "10")
    assert not silent and len(decisions) == T // 1920 - 1 and all(d.startswith("squelch: closed, hold 0,") for d in decisions), decisions[:3]
