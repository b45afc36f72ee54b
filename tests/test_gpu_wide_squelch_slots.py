"""GPU tests of the time-resolved squelch (ABI 620, include/m17hip.h: m17hip_wide_squelch_slots): the three squelch-slot kernels decide per slot of 16 frames
from the group sums spectrum_kernel leaves, and the tile-squelched instantiations of tune_kernel, tune2_kernel and resample_kernel store zeros for a closed
tile and return.  Every comparison is exact: the downloaded float slab, the fetched state words, band powers and tile masks and the meter's planes as uint32
words against the HOST form (tests/squelch_slots_lib.py: detail/core.h under the host compiler over spectrum_lib's group sums and the three tuners' host
forms).  What the host form itself is worth is asserted without a GPU in tests/test_wide_squelch_slots.py.

The layout is tests/test_gpu_wide_squelch.py's: 2 sources, 6 channels — two share a source and a word, one sits on each source's edge word, one listens
between two bins, one never hears anything —, 64 points at hop 64 over low noise.  The tones are switched INSIDE blocks, on slot boundaries.  Blocks: 1020
outputs under wide_config(2, 5) and wide_config2(2, 2, 3) — four tiles of 255, 5 and 6 slots, the last one short — and 1530 under wide_resample(2, 16, 3, 8)
— two tiles of 765 over 64 slots, so one tile spans many.  The integer tuners' block lengths are no multiples of the hop, so `first` varies from block to
block there; the resampler's groups of 8 x 16 samples are whole hops."""
import ctypes as C
import functools

import numpy as np
import pytest

import m17hip
import meter_lib as ml
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_lib as sq
import squelch_slots_lib as ssl
import test_gpu_wide_input as g1
import test_gpu_wide_squelch as g9
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
OPEN = sq.OPEN
FMTS, SB = g1.FMTS, g1.SB
_u32, _assert_words, _dev = g1._u32, g1._assert_words, g1._dev
GAIN = g9.GAIN
POINTS, HOP, HALF = 64, 64, 1
SLOT = 16 * HOP
OPEN_DB, CLOSE_DB = 20.0, 10.0
HANG, LEAD = 1, 1
NBLOCKS = 4
SRC, FCW, AMPL, NAMES = g9.SRC, g9.FCW, g9.AMPL, g9.NAMES
_as_format = g9._as_format


class Kind:
    """One of the three tuners: T outputs per block of Wb samples in tiles of TO, configure(ctx, fmt), tuner(fcw) -> its host form, and `sched`: per block
    the slots [on, off) in which channels 0 and 1 hear their strong tone (None: none)."""


def _kinds():
    out = {}
    k = Kind()
    k.T, k.Wb, k.TO = 1020, 5100, ssl.WIDE_TILE
    taps = m17hip.wide_default_taps(5)
    k.configure = lambda ctx, fmt: ctx.wide_config(2, 5, fmt)
    k.tuner = lambda w: wl.Tuner(taps, 5, w, GAIN)
    k.timer = "tune"
    k.sched = [(4, 5), None, (0, 2), (2, 3)]
    out["config"] = k
    k = Kind()
    k.T, k.Wb, k.TO = 1020, 6120, ssl.WIDE_TILE
    t1, t2 = m17hip.wide_default_taps2(2, 3)
    k.configure = lambda ctx, fmt: ctx.wide_config2(2, 2, 3, fmt)
    k.tuner = lambda w: w2.Tuner2(t1, 2, t2, 3, w, GAIN)
    k.timer = "tune2"
    k.sched = [(5, 6), None, (0, 2), (2, 3)]
    out["config2"] = k
    k = Kind()
    k.T, k.Wb = 1530, 1530 // 3 * 8 * 16
    r1, r2 = m17hip.wide_resample_default_taps(16, 3, 8)
    k.TO = rl.tile_outputs(r1.size, 16, r2.size, 3, 8)
    k.configure = lambda ctx, fmt: ctx.wide_resample(2, 16, 3, 8, fmt)
    k.tuner = lambda w: rl.Resampler(r1, 16, 3, 8, r2, w, GAIN)
    k.timer = "resample"
    k.sched = [(40, 64), None, (0, 2), (32, 33)]
    out["resample"] = k
    return out


KINDS = _kinds()


def _tone(x, s, word, a, b, ampl):
    n = np.arange(a, b)
    x[s, a:b] += ampl * np.exp(2j * np.pi * ((word * n) % (1 << 32)) / float(1 << 32))


def _span(k, b, on, off):
    """The samples of block b's slots [on, off) — to the block's end where `off` is past its last slot."""
    first, J = spl.frames(b * k.Wb, k.Wb, POINTS, HOP)
    G = ssl.slots_stated(J)
    return b * k.Wb + first + on * SLOT, (b + 1) * k.Wb if off >= G else b * k.Wb + first + off * SLOT


@functools.lru_cache(maxsize=None)
def _source(kind, fmt):
    """(data [2][NBLOCKS x Wb] of the format, read-only; the levels (open[2], close[2]) from the host-form plane of a block of the same noise alone).
    Channels 0 and 1 hear the schedule's strong tone; channel 2 a strong one throughout; channel 3 a weak one throughout — between the close and the open
    level — and a strong one in block 1's first two slots, which holds it open from there on; channel 4 a strong one in the middle third of block 2."""
    k = KINDS[kind]
    strong, weak, sigma = AMPL[fmt]
    rng = np.random.default_rng(6200 + len(kind) + 7 * fmt)
    W = NBLOCKS * k.Wb
    x = sigma * (rng.standard_normal((2, W)) + 1j * rng.standard_normal((2, W)))
    for b, ev in enumerate(k.sched):
        if ev is not None:
            _tone(x, 0, FCW[0], *_span(k, b, *ev), strong)
    _tone(x, 0, FCW[2], 0, W, strong)
    _tone(x, 1, FCW[3], 0, W, weak)
    _tone(x, 1, FCW[3], *_span(k, 1, 0, 2), strong)
    _tone(x, 1, FCW[4], 2 * k.Wb + k.Wb // 3, 2 * k.Wb + 2 * k.Wb // 3, strong)
    data = _as_format(x, fmt)
    noise = _as_format(sigma * (rng.standard_normal((2, k.Wb)) + 1j * rng.standard_normal((2, k.Wb))), fmt)
    got = [spl.plane(noise[s], POINTS, HOP) for s in range(2)]
    levels = m17hip.wide_squelch_levels(np.stack([g[0] for g in got]), got[0][1], HALF, OPEN_DB, CLOSE_DB)
    data.setflags(write=False)
    return data, levels


def _feed(kind, data, levels, hang=HANG, lead=LEAD, squelched=True, fcw=FCW):
    k = KINDS[kind]
    feed = ssl.Feed([k.tuner(w) for w in fcw], SRC, data, POINTS, HOP, k.TO)
    if squelched:
        feed.squelch = ssl.SlotSquelch(SRC, fcw, levels[0], levels[1], HALF, hang, lead)
    return feed


@functools.lru_cache(maxsize=None)
def _expected(kind, fmt):
    """The host form of the whole feed of _source: per block (Y, P, U, (state, bands, open, mask, tiles, J)), read-only — and the plan, asserted here on the
    host form before anything runs on the device: channel 0 shows
      a tile open only through the lead, a tile open only through the hang carried from the block before, a closed last tile followed by a block whose
      output 0 is +0 and whose output 1 is not, and an open tile behind a closed one whose first output is the unsquelched word."""
    k = KINDS[kind]
    data, levels = _source(kind, fmt)
    feed = _feed(kind, data, levels)
    out = [feed.block(b * k.Wb, (b + 1) * k.Wb) for b in range(NBLOCKS)]
    tiles = out[0][3][4]
    assert tiles == -(-k.T // k.TO) and all(o[3][4] == tiles for o in out)
    firsts = [spl.frames(b * k.Wb, k.Wb, POINTS, HOP)[0] for b in range(NBLOCKS)]
    assert len(set(firsts)) > 1 or k.Wb % HOP == 0, firsts   # (the resampler's groups are 128 samples: whole hops, `first` stays 0 there)
    flags = [ssl.unpack(o[3][3], tiles)[0] for o in out]
    opens = [o[3][2][0] for o in out]

    def slots_of(b, t, lead):
        a, e = ssl.tile_span_stated(t, k.TO, k.T, k.Wb)
        G = len(opens[b])
        return range(ssl.slot_of_stated(a, firsts[b], HOP, G), min(ssl.slot_of_stated(e - 1, firsts[b], HOP, G) + lead, G - 1) + 1)

    # a tile open only through the lead: none of its own slots is open
    by_lead = [(b, t) for b in range(NBLOCKS) for t in range(tiles) if flags[b][t] and not any(opens[b][g] for g in slots_of(b, t, 0))]
    assert by_lead, (kind, [f.astype(int).tolist() for f in flags])
    # a tile open only through the hang carried from the block before: block 1 hears nothing on the channel, its slot 0 is open, and tile 0 with it
    b1 = out[1][3]
    assert int(out[0][3][0][0]) == (HANG + 1) | OPEN and opens[1][0] and not opens[1][1:].any() and float(b1[1][0, 0]) < float(levels[1][0]) * 16
    assert flags[1][0] and not flags[1][1:].any()
    # block 1's last tile is closed; block 2's output 0 is +0 against the zero carry, its output 1 is not
    assert not flags[1][-1] and flags[2][0] and _u32(out[2][0][0, :1]) == 0 and _u32(out[2][0][0, 1:2]) != 0
    # an open tile behind a closed one: its first output is the unsquelched word (not +0)
    behind = [(b, t) for b in range(NBLOCKS) for t in range(1, tiles) if flags[b][t] and not flags[b][t - 1]]
    assert behind, (kind, [f.astype(int).tolist() for f in flags])
    for b, t in behind:
        assert _u32(out[b][0][0, t * k.TO]) == _u32(out[b][2][0, t * k.TO]) != 0 and (_u32(out[b][0][0, (t - 1) * k.TO:t * k.TO]) == 0).all()
    # the rest of the layout: channel 2 open throughout, channel 5 never, channel 3 held open by its weak tone from block 1 on
    for b, o in enumerate(out):
        f = ssl.unpack(o[3][3], tiles)
        assert f[2].all() and not f[5].any() and np.array_equal(f[0], f[1]) and (f[3].all() if b >= 2 else True) and (not f[3].any() if b == 0 else True)
        assert np.array_equal(_u32(o[0][2]), _u32(o[2][2]))
    for o in out:
        for a in o[:3] + o[3][:4]:
            a.setflags(write=False)
    return out


def _squelch(ctx, levels, hang=HANG, lead=LEAD, half=HALF):
    ctx.wide_squelch_slots(half, levels[0], levels[1], hang, lead)


def _fetch_raw(ctx, back=0, cap=8, capb=8 * 64, capm=8 * 2):
    state, band, mask = np.full(cap, 77, dtype=np.uint32), np.full(capb, 7.0, dtype=np.float32), np.full(capm, 76, dtype=np.uint32)
    n, g, t, frames = C.c_uint32(78), C.c_uint32(79), C.c_uint32(80), C.c_uint32(81)
    code = ctx.lib.m17hip_wide_squelch_slots_fetch(ctx.h, C.c_uint32(back), ol._p(state), ol._p(band), ol._p(mask), C.c_uint64(cap), C.c_uint64(capb),
                                                   C.c_uint64(capm), C.byref(n), C.byref(g), C.byref(t), C.byref(frames))
    assert code == 0 or ((state == 77).all() and (band == 7.0).all() and (mask == 76).all() and (n.value, g.value, t.value, frames.value) == (78, 79, 80, 81))
    return code


def _check_fetch(ctx, exp, what, back=0):
    state, bd, op, mask, tiles, J = exp[3]
    s, b, m, t, frames = ctx.wide_squelch_slots_fetch(back)
    assert (t, frames) == (tiles, J) and s.shape == state.shape and b.shape == bd.shape and m.shape == mask.shape, (what, t, frames, tiles, J, b.shape, bd.shape)
    assert np.array_equal(s, state), (what, s, state)
    _assert_words(b, bd, (what, "bands"))
    assert np.array_equal(m, mask), (what, m, mask)


def _configure(ctx, kind, fmt, fcw=FCW):
    KINDS[kind].configure(ctx, fmt)
    ctx.wide_channels(SRC, fcw)
    ctx.reset()
    ctx.wide_spectrum(POINTS, HOP)


class Uploader(g9.Uploader):
    def __init__(self, ctx, kind, fmt, data, name):
        import torch
        self.ctx, self.k, self.fmt, self.name = ctx, KINDS[kind], fmt, name
        self.Wb = self.k.Wb
        self.host = np.array(data)
        self.W = self.host.shape[1]
        self.dev = _dev(data) if "device" in name else None
        self.pin = torch.from_numpy(self.host).pin_memory() if name == "m17hip_upload_wide_async" else None


# ---- 1: the three tuners, the formats, the ways in ---------------------------------------------------------------------------------------------------------------
CASES = [("config", "i16", NAMES[0]), ("config", "i16", NAMES[1]), ("config", "i16", NAMES[2]), ("config", "i16", NAMES[3]), ("config", "f32", NAMES[2]),
         ("config", "u8", NAMES[2]), ("config2", "i16", NAMES[2]), ("resample", "i16", NAMES[2])]


@pytest.mark.parametrize("kind,fmt,name", CASES)
def test_every_block_is_the_host_forms(kind, fmt, name):
    f = FMTS[fmt]
    data, levels = _source(kind, f)
    exp = _expected(kind, f)
    ctx = m17hip.Context(6, KINDS[kind].T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels)
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
def test_the_meter_on(kind):
    """The same feed with the meter on at window 48: the meter's planes are meter_lib's over the squelched z and y — zeros in closed tiles —, and the
    spectrum's fetch is what it was."""
    f = wl.IQ_I16
    data, levels = _source(kind, f)
    exp = _expected(kind, f)
    k = KINDS[kind]
    Y, P = np.concatenate([e[0] for e in exp], axis=1), np.concatenate([e[1] for e in exp], axis=1)
    ctx = m17hip.Context(6, k.T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels)
        ctx.wide_meter(48)
        up = Uploader(ctx, kind, f, data, NAMES[2])
        for b in range(NBLOCKS):
            up.block(b)
            _assert_words(ctx.download_f32(), exp[b][0], (kind, b))
            _check_fetch(ctx, exp[b], (kind, b))
            planes, fw, fo, t = ctx.wide_meter_fetch()
            assert (fo, t) == (b * k.T, k.T)
            _assert_words(planes, ml.planes(P, Y, b * k.T, (b + 1) * k.T, b * k.T, 48), (kind, b, "meter"))
            power, frames, first = ctx.wide_spectrum_fetch()
            ref = spl.planes(data, POINTS, HOP, [b * k.Wb, (b + 1) * k.Wb])[0]
            assert frames == ref[1] == exp[b][3][5] and first == ref[2]
            _assert_words(power, ref[0], (kind, b, "spectrum"))
    finally:
        ctx.close()


# ---- 2: the mask's word boundary -----------------------------------------------------------------------------------------------------------------------------------
def test_tiles_31_and_32_decide_differently():
    """wide_config(2, 5) at T = 33 x 255 + 7: 34 tiles, two mask words per channel.  Channel 0's tone begins with slot 40 (lead 0): tile 31 — samples
    39 525 to 40 799, slots 38 and 39 — is closed, tile 32 open, and the short tile 33 holds output T - 1."""
    f, kind = wl.IQ_I16, "config"
    T = 33 * 255 + 7
    W = T * 5
    strong, weak, sigma = AMPL[f]
    rng = np.random.default_rng(6203)
    x = sigma * (rng.standard_normal((2, 2 * W)) + 1j * rng.standard_normal((2, 2 * W)))
    _tone(x, 0, FCW[0], 40 * SLOT, W, strong)
    data = _as_format(x, f)
    levels = _source(kind, f)[1]
    feed = _feed(kind, data, levels, hang=0, lead=0)
    exp = [feed.block(0, W), feed.block(W, 2 * W)]
    flags = ssl.unpack(exp[0][3][3], 34)
    assert exp[0][3][4] == 34 and exp[0][3][3].shape == (6, 2) and not flags[0, :32].any() and flags[0, 32:].all() and not flags[2:].any()
    assert not ssl.unpack(exp[1][3][3], 34).any() and (_u32(exp[1][0]) == 0).all()
    ctx = m17hip.Context(6, T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels, 0, 0)
        dev = _dev(data)
        for b in range(2):
            ctx.upload_wide_device(dev.data_ptr() + b * W * 4, 6, T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), exp[b][0], b)
            _check_fetch(ctx, exp[b], b)
    finally:
        ctx.close()


# ---- 3: one slot is the block mode ----------------------------------------------------------------------------------------------------------------------------------
def test_a_block_of_one_slot_at_lead_0_is_the_block_mode_in_the_same_process():
    """wide_config(2, 5), blocks of 200 outputs: 1000 samples, at most 16 frames, one slot and one tile.  The same blocks under m17hip_wide_squelch and under
    m17hip_wide_squelch_slots at lead 0 (hang 1 in either unit): slab, state words and bands are identical."""
    f, kind = wl.IQ_I16, "config"
    data, levels = g9._source(kind, f)
    ctx = m17hip.Context(6, 200)
    try:
        got = {}
        for mode in ("block", "slots"):
            _configure(ctx, kind, f)
            if mode == "block":
                ctx.wide_squelch(HALF, levels[0], levels[1], 1)
            else:
                _squelch(ctx, levels, 1, 0)
            dev = _dev(data)
            got[mode] = []
            for b in range(8):
                ctx.upload_wide_device(dev.data_ptr() + b * 1000 * 4, 6, 200, data.shape[1], GAIN)
                y = ctx.download_f32().copy()
                if mode == "block":
                    o, h, band, frames = ctx.wide_squelch_fetch()
                    state = h | (o.astype(np.uint32) << 31)
                else:
                    state, bands, mask, tiles, frames = ctx.wide_squelch_slots_fetch()
                    assert bands.shape == (6, 1) and tiles == 1 and np.array_equal(mask[:, 0], state >> 31)
                    band = bands[:, 0]
                assert 1 <= frames <= 16
                got[mode].append((y, state, band))
        opened = set()
        for b in range(8):
            for i, what in enumerate(("slab", "state", "band")):
                assert np.array_equal(got["block"][b][i].view(np.uint32), got["slots"][b][i].view(np.uint32)), (b, what)
            opened |= set(((got["block"][b][1] >> 31) != 0).astype(int).tolist())
        assert opened == {0, 1}
    finally:
        ctx.close()


# ---- 4: state ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_block_without_a_frame_is_all_open_and_leaves_the_holds():
    """wide_config at R = 5: a block of 10 outputs is 50 samples, shorter than the 64 points.  Behind block 0 (channel 0 leaves it with a count of 2) it is
    open for every channel with no slot and one tile, the counts stand, and the block behind it finds them."""
    f, kind = wl.IQ_I16, "config"
    k = KINDS[kind]
    data, levels = _source(kind, f)
    feed = _feed(kind, data, levels)
    cuts = [0, k.Wb, k.Wb + 50, 2 * k.Wb + 50]
    exp = [feed.block(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [e[3][5] > 0 for e in exp] == [True, False, True] and exp[1][3][1].shape == (6, 0) and exp[1][3][3].tolist() == [[1]] * 6
    assert int(exp[0][3][0][0]) == 2 | OPEN and int(exp[1][3][0][0]) == 2 | OPEN and int(exp[1][3][0][5]) == OPEN and exp[2][3][2][0, 0]
    ctx = m17hip.Context(6, k.T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels)
        dev = _dev(data)
        for b, T in enumerate((k.T, 10, k.T)):
            ctx.upload_wide_device(dev.data_ptr() + cuts[b] * 4, 6, T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), exp[b][0], b)
            _check_fetch(ctx, exp[b], b)
    finally:
        ctx.close()


def test_resets_a_retune_the_two_modes_and_off():
    """Behind block 0 channels 0 and 1 hold a count of 2.  m17hip_demod_reset_channels([0]) clears channel 0's (and its carry): block 1's tile 0 is closed for
    it and open for channel 1.  A retune of channel 1 keeps its count.  Block mode replaces slot mode and starts the counts over; under it the slot fetch is
    ESTATE, and the other way round; off gives the unsquelched feed and both fetches ESTATE; m17hip_demod_reset clears every count and forgets the planes."""
    f, kind = wl.IQ_I16, "config"
    k = KINDS[kind]
    data, levels = _source(kind, f)
    feed = _feed(kind, data, levels)
    ctx = m17hip.Context(6, k.T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels)
        up = Uploader(ctx, kind, f, data, NAMES[2])

        def both(b, what):
            e = feed.block(b * k.Wb, (b + 1) * k.Wb)
            up.block(b)
            _assert_words(ctx.download_f32(), e[0], what)
            if e[3] is not None:
                _check_fetch(ctx, e, what)
            return e

        e = both(0, "block 0")
        assert (e[3][0][:2] & ~np.uint32(OPEN)).tolist() == [2, 2]
        ctx.reset_channels([0])
        feed.reset([0])
        ctx.wide_channels([0, 0], [FCW[0], FCW[5]])   # (channel 1 to the empty bin of source 0)
        feed.tuners[1].fcw = FCW[5]
        feed.squelch.fcw[1] = FCW[5]
        e = both(1, "block 1: a count cleared, a channel retuned")
        flags = ssl.unpack(e[3][3], e[3][4])
        assert not flags[0].any() and flags[1, 0] and not flags[1, 1:].any()
        assert g9._fetch_raw(ctx) == ESTATE and _fetch_raw(ctx) == 0
        # block mode in its place: the counts start over, the planes are the block mode's
        ctx.wide_squelch(HALF, levels[0], levels[1], 0)
        assert _fetch_raw(ctx) == ESTATE and g9._fetch_raw(ctx) == ESTATE
        plain = sq.Feed(feed.tuners, SRC, data, POINTS, HOP)
        plain.count = feed.count
        plain.squelch = sq.Squelch(SRC, feed.squelch.fcw, levels[0], levels[1], HALF, 0)
        eb = plain.block(2 * k.Wb, 3 * k.Wb)
        up.block(2)
        _assert_words(ctx.download_f32(), eb[0], "block 2: block mode")
        assert g9._fetch_raw(ctx) == 0 and _fetch_raw(ctx) == ESTATE
        o, h, band, frames = ctx.wide_squelch_fetch()
        assert np.array_equal(h | (o.astype(np.uint32) << 31), eb[2])
        # slot mode again: the counts start over once more
        _squelch(ctx, levels)
        assert _fetch_raw(ctx) == ESTATE and g9._fetch_raw(ctx) == ESTATE
        feed.count = plain.count
        feed.squelch = ssl.SlotSquelch(SRC, feed.squelch.fcw, levels[0], levels[1], HALF, HANG, LEAD)
        both(3, "block 3: slot mode again")
        # off, by the slot call and by the block call: the unsquelched feed from the carries as they stand
        ctx.wide_squelch_slots(0, None)
        feed.squelch = None
        assert _fetch_raw(ctx) == ESTATE and g9._fetch_raw(ctx) == ESTATE
        fresh = _feed(kind, data, levels, squelched=False, fcw=[FCW[0], FCW[5]] + FCW[2:])
        e0 = feed.block(0, k.Wb)
        up.block(0)
        _assert_words(ctx.download_f32(), e0[0], "off")
        assert np.array_equal(_u32(e0[0]), _u32(e0[2]))
        _squelch(ctx, levels)
        ctx.wide_squelch(0, None)
        assert _fetch_raw(ctx) == ESTATE
        e1 = feed.block(k.Wb, 2 * k.Wb)
        up.block(1)
        _assert_words(ctx.download_f32(), e1[0], "off by the block mode's call")
        # a reset of the feed with the slot mode on
        _squelch(ctx, levels)
        up.block(0)
        assert _fetch_raw(ctx) == 0
        ctx.reset()
        assert _fetch_raw(ctx) == ESTATE
        fresh.squelch = ssl.SlotSquelch(SRC, [FCW[0], FCW[5]] + FCW[2:], levels[0], levels[1], HALF, HANG, LEAD)
        e = fresh.block(k.Wb, 2 * k.Wb)
        ctx.upload_wide_device(up.dev.data_ptr() + k.Wb * 4, 6, k.T, up.W, GAIN)
        _assert_words(ctx.download_f32(), e[0], "after reset")
        _check_fetch(ctx, e, "after reset")
    finally:
        ctx.close()


def _squelch_raw(ctx, half, o, c, n, hang, lead):
    o = None if o is None else np.ascontiguousarray(o, dtype=np.float32)
    c = None if c is None else np.ascontiguousarray(c, dtype=np.float32)
    return ctx.lib.m17hip_wide_squelch_slots(ctx.h, C.c_uint32(half), None if o is None else ol._p(o), None if c is None else ol._p(c), C.c_uint32(n),
                                             C.c_uint32(hang), C.c_uint32(lead))


def test_state_limits_and_growing_planes():
    f, kind = wl.IQ_I16, "config"
    k = KINDS[kind]
    data, levels = _source(kind, f)
    exp = _expected(kind, f)
    o, c = levels
    ctx = m17hip.Context(6, 4 * k.T)
    try:
        assert _squelch_raw(ctx, 1, o, c, 2, 0, 0) == ESTATE and _squelch_raw(ctx, 0, None, None, 0, 0, 0) == ESTATE   # (no wideband configuration yet)
        k.configure(ctx, f)
        ctx.wide_channels(SRC, FCW)
        ctx.reset()
        assert _squelch_raw(ctx, 1, o, c, 2, 0, 0) == ESTATE   # (the spectrum is off)
        assert _squelch_raw(ctx, 0, None, None, 0, 0, 0) == 0   # (off is off)
        ctx.wide_spectrum(POINTS, HOP)
        for bad in ((65, o, c, 2, 0, 0), (32, o, c, 2, 0, 0), (1, o, c, 2, 65536, 0), (1, o, c, 2, 0, 256), (1, o, c, 1, 0, 0), (1, o, c, 3, 0, 0),
                    (1, o, None, 2, 0, 0), (1, None, c, 2, 0, 0), (1, None, None, 2, 0, 0), (1, o, c, 0, 0, 0), (1, c, o, 2, 0, 0),
                    (1, [np.inf, 1.0], c, 2, 0, 0), (1, o, [0.0, 1.0], 2, 0, 0), (1, [np.nan, 1.0], [np.nan, 1.0], 2, 0, 0)):
            assert _squelch_raw(ctx, *bad) == EINVAL, bad
        assert _squelch_raw(ctx, 31, o, c, 2, 65535, 255) == 0
        _squelch(ctx, levels)
        up = Uploader(ctx, kind, f, data, NAMES[2])
        ctx.timing(True)
        ctx.timing_reset()
        before = ctx.iq_bytes()
        up.block(0)
        _check_fetch(ctx, exp[0], "block 0")
        assert _fetch_raw(ctx) == 0 and _fetch_raw(ctx, 1) == ESTATE and _fetch_raw(ctx, 2) == EINVAL
        assert _fetch_raw(ctx, 0, cap=5) == EINVAL and _fetch_raw(ctx, 0, capb=29) == EINVAL and _fetch_raw(ctx, 0, capm=5) == EINVAL
        assert ctx.lib.m17hip_wide_squelch_slots_fetch(ctx.h, C.c_uint32(0), None, None, None, C.c_uint64(8), C.c_uint64(512), C.c_uint64(16), None, None, None,
                                                       None) == EINVAL
        small = ctx.iq_bytes()
        assert small >= before + (6 * 5 + 6 + 6) * 4
        ms, launches = ctx.timing_get("squelch_slots")
        assert launches == 1 and ms > 0.0 and ctx.timing_get("squelch")[1] == 0 and ctx.timing_get("tune")[1] == 1 and ctx.timing_get("spectrum")[1] == 1
        ctx.timing(False)
        # a block four times as long: the planes regrow, and the block before's are still there for back = 1
        feed = _feed(kind, data, levels)
        feed.block(0, k.Wb)
        e = feed.block(0, 4 * k.Wb)
        ctx.upload_wide_device(up.dev.data_ptr(), 6, 4 * k.T, up.W, GAIN)
        _assert_words(ctx.download_f32(), e[0], "the long block")
        _check_fetch(ctx, e, "the long block")
        _check_fetch(ctx, exp[0], "the short one before it", back=1)
        assert e[3][1].shape[1] > 3 * exp[0][3][1].shape[1] and ctx.iq_bytes() > small
        # every m17hip_wide_spectrum call and every configuration call turns it off
        ctx.wide_spectrum(POINTS, HOP)
        assert _fetch_raw(ctx) == ESTATE
        for conf in (lambda: ctx.wide_config(2, 5), lambda: ctx.wide_config2(2, 2, 3), lambda: ctx.wide_resample(2, 16, 3, 8), lambda: ctx.wide_raster(2, 5, 48)):
            _configure(ctx, kind, f)
            _squelch(ctx, levels)
            up.block(0)
            assert _fetch_raw(ctx) == 0
            conf()
            assert _fetch_raw(ctx) == ESTATE
        ctx.wide_spectrum(POINTS, HOP)
        assert _squelch_raw(ctx, 1, o, c, 2, 0, 0) == ESTATE and _squelch_raw(ctx, 0, None, None, 0, 0, 0) == 0   # (under a raster)
    finally:
        ctx.close()


# ---- 5: two blocks in flight ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_staged_and_an_in_place_block_in_flight_then_a_run(kind):
    """Block 0 staged on the copy stream, block 1 in place on the main stream, no wait in between, then the staged block's run: back = 1 and back = 0 are each
    their own host form — the hold counts, the slots' flags and the carries cross the streams behind ev_iq —, and the slab the run worked on is the staged
    block's."""
    f = wl.IQ_I16
    data, levels = _source(kind, f)
    exp = _expected(kind, f)
    T = KINDS[kind].T
    ctx = m17hip.Context(6, T)
    try:
        _configure(ctx, kind, f)
        _squelch(ctx, levels)
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


# ---- 6: the example ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_example_keeps_a_transmission_that_begins_inside_a_block_and_prints_nothing_for_an_empty_offset():
    """examples/m17-demod-gpu --spectrum 2048 --squelch 10 --slots --lead 1 --hang 1 on tests/test_wide_squelch_slots.py's source with 100 ms of noise in
    front: the example's blocks are 1920 outputs (40 ms), the first runs unsquelched and sets the levels, the second is noise alone, and the transmission
    begins in the middle of the third.  Tuned to the transmission it prints the lines of the unsquelched run, with fewer tiles open than there are; tuned to
    empty spectrum it prints no frame and opens no tile.  (The noise in front is kept short on the demodulator's account, not the squelch's: its carrier
    detect reads a long run of exact zeros — 19 000 were measured, 16 000 were not — as a carrier and false-locks on the edge behind it.)"""
    import os
    import re
    import subprocess
    import test_wide_squelch_slots as cpu
    bb, row = cpu._late_transmission(1600 * 128)
    exe = os.path.join(wl.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    raw = np.ascontiguousarray(row).tobytes()

    def run(offset, *more):
        r = subprocess.run([exe, "--wide-i16", "--rate", "2048000", "--offset-hz", str(offset), "--spectrum", "2048", *more], input=raw, capture_output=True,
                           check=True, timeout=120)
        tiles = [tuple(int(v) for v in re.match(r"squelch: (\d+) of (\d+) tiles open", l).groups()) for l in r.stderr.decode().split("\n") if l.startswith("squelch:")]
        return [l for l in r.stdout.decode().split("\n") if l.strip()], tiles

    plain, none = run(12500)
    kept, tiles = run(12500, "--squelch", "10", "--slots", "--lead", "1", "--hang", "1")
    assert len(plain) >= 6 and kept == plain and not none
    assert tiles and 0 < sum(a for a, b in tiles) < sum(b for a, b in tiles), tiles
    silent, tiles = run(-600000, "--squelch", "10", "--slots", "--lead", "1")
    assert not silent and tiles and not any(a for a, b in tiles), tiles
