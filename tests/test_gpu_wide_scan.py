"""GPU tests of the carrier scan (ABI 622, include/m17hip.h: m17hip_wide_scan): wide_scan_kernel finds the carriers of each source's block in the block's own
spectrum plane and writes the frequency words of the source's pool of channels; the block's unchanged squelch kernel and tuner read the table it leaves.  Every
comparison is exact on words against the HOST form (tests/scan_lib.py over squelch_floor_lib and squelch_lib): the fetched table, flags and misses, the floor
plane, the state words, the bands, the output slabs and the meter planes.  What the host form itself is worth is asserted without a GPU in
tests/test_wide_scan.py.

The layout: 3 sources, 10 channels, 64 points at hop 64 under a rectangular window, a band of 3 bins, a guard of 4, 6 / 3 dB, hang 1.  Source 0 (slots 0 - 2,
channel 3 fixed on its first carrier): noise with carriers in bins 10 and 30 throughout and in bin 50 in blocks 2 and 3.  Source 1 (slots 4 and 5, channel 6
fixed on an empty bin): noise with carriers in bins 8, 24 and 40 — one more than it has slots.  Source 2 (slots 7 and 8, channel 9 fixed) is made of exact
samples: zeros; one impulse at a frame start (a spectrum flat to the bit: every bin ties); zeros; a NaN sample (float32; the other formats a second
impulse); two on-bin tones; zeros."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import meter_lib as ml
import oracle_lib as ol
import resample_lib as rl
import scan_lib as sc
import squelch_floor_lib as sf
import squelch_lib as sq
import test_gpu_wide_input as g1
import test_gpu_wide_squelch as g9
import test_resample_input as tr
import test_wide_scan as t22
import test_wide_squelch_floor as t21
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ETRUNC = -1, -4, -6
OPEN = sq.OPEN
SLOT, ASSIGNED, HELD = sc.SLOT, sc.ASSIGNED, sc.HELD
_u32, _assert_words, _dev = g1._u32, g1._assert_words, g1._dev
FMTS, SB, GAIN, NAMES = g9.FMTS, g9.SB, g9.GAIN, g9.NAMES
POINTS, HOP, HALF, GUARD, HANG = 64, 64, 1, 4, 1
WIN = np.ones(POINTS, dtype=np.float32)
RO, RC = m17hip.wide_squelch_ratio(6.0), m17hip.wide_squelch_ratio(3.0)
NBLOCKS = 6
SRC = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
POOL = [1, 1, 1, 0, 1, 1, 0, 1, 1, 0]
BINS = [60, 60, 60, 10, 60, 60, 33, 5, 6, 16]
FCW = [t22._word(k, POINTS) for k in BINS]
CH = len(SRC)
AMPL = {wl.IQ_I16: (5000.0, 20.0), wl.IQ_F32: (5000.0, 20.0), wl.IQ_U8: (40.0, 6.0)}   # carrier, noise sigma per component (uint8: nothing clips, and the noise dithers the rounding)


class Kind:
    """One of the three tuners: T outputs (a multiple of 192: the listed reset's rule) per block of Wb samples, configure(ctx, fmt, sources), tuner(fcw)."""


def _kinds():
    out = {}
    k = Kind()
    k.T, k.Wb = 384, 1920       # (two tiles of 255 outputs)
    taps = m17hip.wide_default_taps(5)
    k.configure = lambda ctx, fmt, S=3: ctx.wide_config(S, 5, fmt)
    k.tuner = lambda w: wl.Tuner(taps, 5, w, GAIN)
    out["config"] = k
    k = Kind()
    k.T, k.Wb = 192, 768        # (one tile)
    t1, t2 = m17hip.wide_default_taps2(2, 2)
    k.configure = lambda ctx, fmt, S=3: ctx.wide_config2(S, 2, 2, fmt)
    k.tuner = lambda w: w2.Tuner2(t1, 2, t2, 2, w, GAIN)
    out["config2"] = k
    k = Kind()
    r1, r2 = wl.hamming_taps(33), (3 * wl.hamming_taps(65).astype(np.float64)).astype(np.float32)   # (short taps: tests/test_resample_input.py's TILES)
    k.T = 1536                  # (three tiles of rl.tile_outputs, the last of 6 outputs: asserted below)
    k.Wb = k.T // 3 * 8 * 16
    k.configure = lambda ctx, fmt, S=3: ctx.wide_resample(S, 16, 3, 8, fmt, r1, r2)
    k.tuner = lambda w: rl.Resampler(r1, 16, 3, 8, r2, w, GAIN)
    out["resample"] = k
    return out


KINDS = _kinds()


def _tone(x, s, k, a, b, ampl, N=POINTS):
    n = np.arange(a, b)
    x[s, a:b] += ampl * np.exp(2j * np.pi * ((k * n) % N) / float(N))


@functools.lru_cache(maxsize=None)
def _source(kind, fmt):
    """data [3][NBLOCKS x Wb] of the format, read-only."""
    k = KINDS[kind]
    strong, sigma = AMPL[fmt]
    rng = np.random.default_rng(6220 + len(kind) + 7 * fmt)
    Wb, W = k.Wb, NBLOCKS * k.Wb
    assert Wb % HOP == 0
    x = sigma * (rng.standard_normal((3, W)) + 1j * rng.standard_normal((3, W)))
    x[2] = 0.0
    for kb in (10, 30):
        _tone(x, 0, kb, 0, W, strong)
    _tone(x, 0, 50, 2 * Wb, 4 * Wb, strong)
    for kb, a in ((8, 1.0), (24, 0.7), (40, 0.4)):
        _tone(x, 1, kb, 0, W, a * strong)
    x[2, Wb + 3 * HOP] = strong                                   # (block 1: an impulse at a frame start)
    if fmt != wl.IQ_F32:
        x[2, 3 * Wb + 5 * HOP] = complex(0.0, strong)
    n = np.arange(4 * Wb, 5 * Wb)
    x[2, 4 * Wb:5 * Wb] = (strong / 4) * ((1j) ** (n % 4) + (-1.0) ** (n % 2))   # (block 4: bins 16 and 32, exact samples)
    data = g9._as_format(x, fmt)
    if fmt == wl.IQ_F32:
        data[2, 3 * Wb + 5 * HOP + 7] = np.complex64(complex(np.nan, 1.0))
    data.setflags(write=False)
    return data


def _feed(kind, data, src=SRC, fcw=FCW, pool=POOL, sources=3, points=POINTS, hop=HOP, win=WIN, half=HALF, guard=GUARD, hang=HANG, auto=False):
    k = KINDS[kind]
    feed = sc.Feed([k.tuner(w) for w in fcw], src, data, points, hop, win)
    feed.squelch = sq.Squelch(src, fcw, np.ones(sources), np.ones(sources), half, hang)
    feed.floor = sf.Floor(sources, half, RO, RC)
    feed.scan = sc.Scan(pool, guard, fcw)
    feed.auto_reset = auto
    return feed


def _freeze(e):
    for a in e:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _expected(kind, fmt, auto):
    """The host form of the whole feed: per block (Y, P, state, band, J, floor, words, flags, missed); `auto`: the assigned channels reset behind each block,
    as Context.run() does.  The plan is asserted on it before anything runs on the device."""
    k = KINDS[kind]
    feed = _feed(kind, _source(kind, fmt), auto=auto)
    out = [_freeze(feed.block(b * k.Wb, (b + 1) * k.Wb)) for b in range(NBLOCKS)]
    new = np.array([(e[7] & ASSIGNED) != 0 for e in out]).astype(int)
    held = np.array([(e[7] & HELD) != 0 for e in out]).astype(int)
    missed = np.array([e[8] for e in out])
    assert new[:, :3].sum(axis=1).tolist() == [2, 0, 1, 0, 0, 0] and held[3, :3].tolist() == [1, 1, 1], (kind, fmt, new, held)   # (bin 50 comes and goes)
    assert new[0, 4:6].tolist() == [1, 1] and not new[1:, 4:6].any() and missed[:, 1].tolist() == [1] * NBLOCKS, (kind, fmt, missed)  # (one carrier too many)
    assert not new[:, [3, 6, 9]].any() and all((e[7][[3, 6, 9]] == 0).all() for e in out)
    bins = [sq.bin_stated(int(w), 6) for w in out[3][6][:3]]
    assert sorted(bins) == [10, 30, 50], bins
    if fmt == wl.IQ_U8:   # (uint8 has no zero: 127.5 rounds to 128, so its "zeros" are a carrier of half a unit at bin 0, which the host form takes as it is)
        return out
    # the zeros: levels of +0, every bin ties at them, bin 0 is the one peak and the slots, held on bins 5 and 6, do not cover it.  The impulse: a plane flat to
    # the bit, the median is every bin's word, every band ties BELOW the open level: no peak, and the slots are held by their hang time
    assert missed[0, 2] == 1 and held[0, 7:9].tolist() == [1, 1] and out[0][5][0, 2] == 0
    assert out[1][5][0, 2] > 0 and held[1, 7:9].tolist() == [1, 1] and missed[1, 2] == 0 and not (out[1][2][7:9] & ~np.uint32(OPEN) == HANG + 1).any()
    if fmt == wl.IQ_F32:
        assert np.isnan(out[3][5][0, 2]) and (out[3][7][7:9] == SLOT).all()   # (the NaN sample: the scan is idle on that source)
    # the two tones on exact zeros: the median and so the levels are +0, both slots are held where they stand, and bin 0 ties its way to a peak beside the tones'
    assert held[4, 7:9].tolist() == [1, 1] and missed[4, 2] == 3 and out[4][5][0, 2] == 0
    return out


def _configure(ctx, kind, fmt, src=SRC, fcw=FCW, pool=POOL, sources=3, points=POINTS, hop=HOP, win=WIN, half=HALF, guard=GUARD, hang=HANG, scan=True):
    KINDS[kind].configure(ctx, fmt, sources)
    ctx.wide_channels(src, fcw)
    ctx.reset()
    ctx.wide_spectrum(points, hop, win)
    ctx.wide_squelch(half, np.ones(sources, dtype=np.float32), np.ones(sources, dtype=np.float32), hang)
    ctx.wide_squelch_floor(RO, RC)
    if scan:
        ctx.wide_scan(pool, guard)


def _check(ctx, e, what, back=0):
    Y, P, state, band, J, floor, words, flags, missed = e
    n = state.size
    g9._check_fetch(ctx, (Y, P, state, band, J), what, back)
    plane, frames = ctx.wide_squelch_floor_fetch(back)
    assert frames == J
    _assert_words(plane, floor, (what, "floor plane"))
    w, f, m, assigned = ctx.wide_scan_fetch(back)
    assert np.array_equal(w, words[:n]), (what, "words", w, words)
    assert np.array_equal(f, flags[:n]), (what, "flags", f, flags)
    assert np.array_equal(m, missed), (what, "missed", m, missed)
    assert assigned == [int(c) for c in np.flatnonzero(flags[:n] & ASSIGNED)]


class Up:
    """One of the four entry points over the blocks of one feed; a staged block is run through Context.run(), which resets what the block assigned."""

    def __init__(self, ctx, kind, fmt, data, name):
        import torch
        self.ctx, self.k, self.fmt, self.name = ctx, KINDS[kind], fmt, name
        self.host = np.array(data)
        self.W = self.host.shape[1]
        self.dev = _dev(data) if "device" in name else None
        self.pin = torch.from_numpy(self.host).pin_memory() if name == "m17hip_upload_wide_async" else None

    def block(self, b, channels=CH, run=True):
        off = b * self.k.Wb * SB[self.fmt]
        base = self.dev.data_ptr() if self.dev is not None else self.pin.data_ptr() if self.pin is not None else self.host.ctypes.data
        self.ctx._upload_wide_raw(self.name, base + off, channels, self.k.T, self.W, GAIN)
        if self.name.endswith("_async") and run:
            self.ctx.run(channels=channels, samples=self.k.T)


def _scan_raw(ctx, pool, n, guard):
    a = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint8)
    return ctx.lib.m17hip_wide_scan(ctx.h, None if a is None else ol._p(a), C.c_uint32(n), C.c_uint32(guard))


def _fetch_raw(ctx, back=0, cap=CH, null=False):
    fcw, flags, missed = np.full(max(cap, 1), 7, dtype=np.int32), np.full(max(cap, 1), 7, dtype=np.uint32), np.full(256, 7, dtype=np.uint32)
    n, s, j = C.c_uint32(77), C.c_uint32(78), C.c_uint32(79)
    code = ctx.lib.m17hip_wide_scan_fetch(ctx.h, C.c_uint32(back), None if null else ol._p(fcw), ol._p(flags), ol._p(missed), C.c_uint64(cap), C.byref(n),
                                          C.byref(s), C.byref(j))
    if code not in (0, ETRUNC):   # (a refusal writes nothing)
        assert (fcw == 7).all() and (flags == 7).all() and (missed == 7).all() and (n.value, s.value, j.value) == (77, 78, 79)
    return code, fcw, flags, n.value


# ---- 1: the three tuners, the three formats, the four ways in -------------------------------------------------------------------------------------------------
def test_the_resampling_kind_has_three_tiles_a_block():
    k = KINDS["resample"]
    TO = rl.tile_outputs(33, 16, 65, 3, 8)
    assert 2 * TO < k.T <= 3 * TO, TO


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", ("i16", "f32", "u8"))
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_block_is_the_host_forms(kind, fmt, name):
    f = FMTS[fmt]
    k = KINDS[kind]
    data = _source(kind, f)
    staged = name.endswith("_async")
    exp = _expected(kind, f, staged)
    Y, P = np.concatenate([e[0] for e in exp], axis=1), np.concatenate([e[1] for e in exp], axis=1)
    ctx = m17hip.Context(CH, k.T)
    try:
        _configure(ctx, kind, f)
        ctx.wide_meter(48)
        assert _fetch_raw(ctx)[0] == ESTATE
        up = Up(ctx, kind, f, data, name)
        for b in range(NBLOCKS):
            up.block(b)
            _assert_words(ctx.download_f32(), exp[b][0], (kind, fmt, name, b))
            _check(ctx, exp[b], (kind, fmt, name, b))
            if b:
                _check(ctx, exp[b - 1], (kind, fmt, name, b, "back"), back=1)
            else:
                assert _fetch_raw(ctx, 1)[0] == ESTATE
            planes, fw, fo, t = ctx.wide_meter_fetch()
            assert (fo, t) == (b * k.T, k.T)
            _assert_words(planes, ml.planes(P, Y, b * k.T, (b + 1) * k.T, b * k.T, 48), (kind, fmt, name, b, "meter"))
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 2: 4096 points -----------------------------------------------------------------------------------------------------------------------------------------------
BIG, BIG_T, BIG_X = 4096, 2496, 154   # (12 480 samples a block: two frames at the least; the guard of 9 kHz at 240 kSPS)
BIG_SRC = [0, 0, 0, 0, 1, 1, 1, 1]
BIG_POOL = [1, 1, 1, 0, 1, 1, 1, 0]
BIG_BINS = [2000, 2000, 2000, 700, 100, 100, 100, 3000]
BIG_AT = {0: (700, 1500, 3900), 1: (40, 200, 2048, 4090)}   # (source 1: one carrier more than slots, and two across the wrap, 46 bins apart: one peak)


@functools.lru_cache(maxsize=None)
def _big():
    W = BIG_T * 5
    rng = np.random.default_rng(62204)
    x = 20.0 * (rng.standard_normal((2, 2 * W)) + 1j * rng.standard_normal((2, 2 * W)))
    for s, at in BIG_AT.items():
        for i, kb in enumerate(at):
            _tone(x, s, kb, 0, 2 * W, 3000.0 - 300.0 * i, BIG)
    data = g9._as_format(x, wl.IQ_I16)
    data.setflags(write=False)
    fcw = [t22._word(k, BIG) for k in BIG_BINS]
    taps = m17hip.wide_default_taps(5)
    feed = sc.Feed([wl.Tuner(taps, 5, w, GAIN) for w in fcw], BIG_SRC, data, BIG, BIG)
    feed.squelch = sq.Squelch(BIG_SRC, fcw, np.ones(2), np.ones(2), 4, HANG)
    feed.floor = sf.Floor(2, 4, RO, RC)
    feed.scan = sc.Scan(BIG_POOL, BIG_X, fcw)
    exp = [_freeze(feed.block(b * W, (b + 1) * W)) for b in range(2)]
    assert all(e[4] >= 2 for e in exp)
    assert (exp[0][7][:3] == SLOT | ASSIGNED).all() and exp[0][8].tolist() == [0, 0] and (exp[1][7][:3] == SLOT | HELD).all()
    assert int((exp[0][7][4:7] & ASSIGNED != 0).sum()) == 3 and (exp[1][7][4:7] == SLOT | HELD).all()   # (4090 and 40 are one peak: three peaks, three slots)
    return data, fcw, exp


def test_4096_points():
    data, fcw, exp = _big()
    W = BIG_T * 5
    ctx = m17hip.Context(8, BIG_T)
    try:
        ctx.wide_config(2, 5, wl.IQ_I16)
        ctx.wide_channels(BIG_SRC, fcw)
        ctx.reset()
        ctx.wide_spectrum(BIG, BIG)
        ctx.wide_squelch(4, np.ones(2, dtype=np.float32), np.ones(2, dtype=np.float32), HANG)
        ctx.wide_squelch_floor(RO, RC)
        ctx.wide_scan(BIG_POOL)   # (the default guard: 9 kHz at the configuration's 240 kSPS)
        dev = _dev(data)
        for b in range(2):
            ctx.upload_wide_device(dev.data_ptr() + b * W * 4, 8, BIG_T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), exp[b][0], b)
            _check(ctx, exp[b], ("4096", b))
    finally:
        ctx.close()


# ---- 3: 256 sources of one slot each; 256 slots on one source --------------------------------------------------------------------------------------------------
def _wide_case(S, src, pool, fcw, at, blocks=2, T=192):
    """float32 sources of noise and on-bin carriers `at[s]`; -> (data, expected)."""
    Wb = T * 5
    rng = np.random.default_rng(62205 + S)
    x = 20.0 * (rng.standard_normal((S, blocks * Wb)) + 1j * rng.standard_normal((S, blocks * Wb)))
    for s in range(S):
        for i, kb in enumerate(at(s)):
            _tone(x, s, kb, 0, blocks * Wb, 5000.0 - 100.0 * i)
    data = x.astype(np.complex64)
    k = KINDS["config"]
    feed = sc.Feed([k.tuner(w) for w in fcw], src, data, POINTS, HOP, WIN)
    feed.squelch = sq.Squelch(src, fcw, np.ones(S), np.ones(S), HALF, HANG)
    feed.floor = sf.Floor(S, HALF, RO, RC)
    feed.scan = sc.Scan(pool, GUARD, fcw)
    return data, [feed.block(b * Wb, (b + 1) * Wb) for b in range(blocks)]


def _run_case(S, src, pool, fcw, data, exp, T=192):
    n = len(src)
    ctx = m17hip.Context(n, T)
    try:
        _configure(ctx, "config", wl.IQ_F32, src, fcw, pool, S)
        dev = _dev(data)
        for b, e in enumerate(exp):
            ctx.upload_wide_device(dev.data_ptr() + b * T * 5 * 8, n, T, data.shape[1], GAIN)
            _assert_words(ctx.download_f32(), e[0], b)
            _check(ctx, e, (S, b))
    finally:
        ctx.close()


def test_256_sources_of_one_slot_each():
    S = 256
    src, pool, fcw = list(range(S)), [1] * S, [t22._word(60, POINTS)] * S
    data, exp = _wide_case(S, src, pool, fcw, lambda s: (5 + s % 50,))
    assert (exp[0][7] == SLOT | ASSIGNED).all() and (exp[1][7] == SLOT | HELD).all() and not exp[0][8].any()
    assert [sq.bin_stated(int(w), 6) for w in exp[0][6]] == [5 + s % 50 for s in range(S)]
    _run_case(S, src, pool, fcw, data, exp)


def test_256_slots_on_one_source_and_one_more_is_refused():
    n = 256
    src, pool, fcw = [0] * n, [1] * n, [t22._word(61, POINTS)] * n
    data, exp = _wide_case(1, src, pool, fcw, lambda s: (5, 15, 25, 35, 45, 55))
    new = (exp[0][7] & ASSIGNED) != 0
    assert new[:6].all() and not new[6:].any() and [sq.bin_stated(int(w), 6) for w in exp[0][6][:6]] == [5, 15, 25, 35, 45, 55]
    _run_case(1, src, pool, fcw, data, exp)
    ctx = m17hip.Context(n + 1, 192)
    try:
        _configure(ctx, "config", wl.IQ_F32, [0] * (n + 1), fcw + fcw[:1], [1] * (n + 1), 1)
        dev = _dev(data)
        assert g1._raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), n + 1, 192, data.shape[1], GAIN) == ESTATE   # (257 slots among the block's channels)
        assert g1._raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), n, 192, data.shape[1], GAIN) == 0            # (256 of them: the table in force per block)
        w, f, m, assigned = ctx.wide_scan_fetch()
        assert assigned == list(range(6)) and w.size == n
    finally:
        ctx.close()


# ---- 4: two blocks in flight on alternating streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_six_blocks_two_in_flight(kind):
    """Blocks 0, 2, 4 staged on the copy stream, blocks 1, 3, 5 in place on the main stream with no wait in between, then the staged block's run (the library's
    own call: nothing is reset): back = 1 and back = 0 are each their own host form — the slots' words, the hold counts and the floor cross the streams behind
    ev_iq —, and the slab the run worked on is the staged block's."""
    f = wl.IQ_I16
    k = KINDS[kind]
    data = _source(kind, f)
    exp = _expected(kind, f, False)
    ctx = m17hip.Context(CH, k.T)
    try:
        _configure(ctx, kind, f)
        staged, inplace = Up(ctx, kind, f, data, NAMES[3]), Up(ctx, kind, f, data, NAMES[2])
        inplace.dev = staged.dev
        for b in range(0, NBLOCKS, 2):
            staged.block(b, run=False)
            inplace.block(b + 1)
            _check(ctx, exp[b], (kind, b, "staged"), back=1)
            _check(ctx, exp[b + 1], (kind, b + 1, "in place"), back=0)
            ctx._chk(ctx.lib.m17hip_demod_run(ctx.h, C.c_uint32(CH), C.c_uint32(k.T), C.c_uint32(0)))
            _assert_words(ctx.download_f32(), exp[b][0], (kind, b, "the staged block's slab"))
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: against the paths that exist ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_fetched_table_given_through_wide_channels_and_the_scan_off(kind):
    """A second context with no scan, given each block's fetched table through m17hip_wide_channels in front of the block: the same slabs, state words and
    bands.  And a context whose scan was on and is turned off gives what one gives that never had it."""
    f = wl.IQ_I16
    k = KINDS[kind]
    data = _source(kind, f)
    exp = _expected(kind, f, False)
    a, b_, c_ = m17hip.Context(CH, k.T), m17hip.Context(CH, k.T), m17hip.Context(CH, k.T)
    try:
        _configure(a, kind, f)
        _configure(b_, kind, f, scan=False)
        _configure(c_, kind, f)
        dev = _dev(data)
        for b in range(NBLOCKS):
            a.upload_wide_device(dev.data_ptr() + b * k.Wb * SB[f], CH, k.T, data.shape[1], GAIN)
            words = a.wide_scan_fetch()[0]
            assert np.array_equal(words, exp[b][6])
            b_.wide_channels(SRC, words)
            b_.upload_wide_device(dev.data_ptr() + b * k.Wb * SB[f], CH, k.T, data.shape[1], GAIN)
            _assert_words(b_.download_f32(), a.download_f32(), (kind, b, "given table"))
            sa, sb = a.wide_squelch_fetch(), b_.wide_squelch_fetch()
            assert all(np.array_equal(_u32(x) if x.dtype == np.float32 else x, _u32(y) if y.dtype == np.float32 else y) for x, y in zip(sa[:3], sb[:3]))
        # off: c_ has uploaded a scanned block, then turns the scan off; b_ never had one; both start over and see the host's table
        c_.upload_wide_device(dev.data_ptr(), CH, k.T, data.shape[1], GAIN)
        c_.wide_scan(None)
        assert _fetch_raw(c_)[0] == ESTATE
        b_.wide_channels(SRC, FCW)
        for ctx in (b_, c_):
            ctx.reset()
        for b in range(2):
            for ctx in (b_, c_):
                ctx.upload_wide_device(dev.data_ptr() + b * k.Wb * SB[f], CH, k.T, data.shape[1], GAIN)
            _assert_words(c_.download_f32(), b_.download_f32(), (kind, b, "scan off"))
            assert np.array_equal(c_.wide_squelch_fetch()[1], b_.wide_squelch_fetch()[1])
    finally:
        for ctx in (a, b_, c_):
            ctx.close()


# ---- 6: state and limits ------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_and_limits():
    kind, f = "config", wl.IQ_I16
    k = KINDS[kind]
    data = _source(kind, f)
    dev = _dev(data)
    ones = np.ones(3, dtype=np.float32)
    ctx = m17hip.Context(CH, k.T)
    try:
        assert _scan_raw(ctx, POOL, CH, GUARD) == ESTATE                       # (no wideband configuration)
        k.configure(ctx, f, 3)
        ctx.wide_channels(SRC, FCW)
        ctx.reset()
        assert _scan_raw(ctx, POOL, CH, GUARD) == ESTATE                       # (no spectrum)
        ctx.wide_spectrum(POINTS, HOP, WIN)
        assert _scan_raw(ctx, POOL, CH, GUARD) == ESTATE                       # (no squelch)
        ctx.wide_squelch(HALF, ones, ones, HANG)
        assert _scan_raw(ctx, POOL, CH, GUARD) == ESTATE                       # (no floor)
        ctx.wide_squelch_slots(HALF, ones, ones, HANG, 0)
        ctx.wide_squelch_floor(RO, RC)
        assert _scan_raw(ctx, POOL, CH, GUARD) == ESTATE                       # (the slot mode)
        assert _scan_raw(ctx, None, 0, 0) == 0                                 # (off while off)
        ctx.wide_squelch(HALF, ones, ones, HANG)
        ctx.wide_squelch_floor(RO, RC)
        for pool, n, x in ((POOL, CH, 2), (POOL, CH, POINTS // 4 + 1), (POOL, CH + 1, GUARD), (None, CH, GUARD), (POOL, 0, GUARD)):
            assert _scan_raw(ctx, pool, n, x) == EINVAL, (n, x)
        assert _scan_raw(ctx, POOL, CH, POINTS // 4) == 0 and _scan_raw(ctx, POOL, CH, 3) == 0 and _scan_raw(ctx, POOL, CH, GUARD) == 0
        assert _fetch_raw(ctx)[0] == ESTATE                                    # (no block yet)
        ctx.upload_wide_device(dev.data_ptr(), CH, k.T, data.shape[1], GAIN)
        assert _fetch_raw(ctx, 2)[0] == EINVAL and _fetch_raw(ctx, 0, null=True)[0] == EINVAL and _fetch_raw(ctx, 1)[0] == ESTATE
        code, fcw, flags, n = _fetch_raw(ctx, 0, cap=4)                        # (truncated: the first four, and the count)
        exp = _expected(kind, f, False)[0]
        assert code == ETRUNC and n == CH and np.array_equal(fcw, exp[6][:4]) and np.array_equal(flags, exp[7][:4])
        # a slot stays with its source; every other entry may change, a slot's word included (its seed)
        moved = list(SRC)
        moved[1] = 1
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(np.array(moved, dtype=np.uint32)), ol._p(np.array(FCW, dtype=np.int32)), C.c_uint32(CH)) == ESTATE
        moved = list(SRC)
        moved[3] = 2
        ctx.wide_channels(moved, [0] * CH)
        ctx.wide_channels(SRC, FCW)
        # what turns it off
        for off in (lambda: ctx.wide_squelch_floor(0.0, 0.0), lambda: ctx.wide_squelch(HALF, ones, ones, HANG), lambda: ctx.wide_squelch(0, None),
                    lambda: ctx.wide_spectrum(POINTS, HOP, WIN), lambda: k.configure(ctx, f, 3)):
            off()
            assert _fetch_raw(ctx)[0] == ESTATE
            if not ctx.lib.m17hip_version() or _scan_raw(ctx, POOL, CH, GUARD) != 0:   # (back on where the rest still stands; otherwise all of it again)
                _configure(ctx, kind, f)
            ctx.upload_wide_device(dev.data_ptr(), CH, k.T, data.shape[1], GAIN)
            assert _fetch_raw(ctx)[0] == 0
    finally:
        ctx.close()


# ---- 7: through the whole chain -------------------------------------------------------------------------------------------------------------------------------------
def test_three_transmissions_through_the_scanned_resampler_and_the_whole_chain():
    """The 2.048 MSPS source of three transmissions in 100 ms blocks, four slots seeded at +400 kHz (tests/test_wide_scan.py has the host form and what it
    shows).  Context.run() resets the channels block 0 assigns; the records of every run are the float oracle's on the host form's floats."""
    blocks, seed, B, X = t22.three()
    bb, x = t21._source()
    cuts = t21._cuts(x.shape[0])
    T = t21.BLOCK
    ctx = m17hip.Context(4, T)
    recs = []
    try:
        ctx.wide_resample(1, tr.CH_R1, tr.CH_U, tr.CH_D)
        ctx.wide_channels([0] * 4, [seed] * 4)
        ctx.reset()
        ctx.wide_spectrum(t21.POINTS, t21.HOP)
        ctx.wide_squelch(B, [1.0], [1.0], t21.HANG)
        ctx.wide_squelch_floor(m17hip.wide_squelch_ratio(t21.OPEN_DB), m17hip.wide_squelch_ratio(t21.CLOSE_DB))
        ctx.wide_scan([1] * 4, rate_hz=t21.RATE)
        for (a, b), e in zip(cuts, blocks):
            n = (b - a) // (tr.CH_R1 * tr.CH_D) * tr.CH_U
            ctx.upload_wide(x[None, a:b], channels=4)
            w, f, m, assigned = ctx.wide_scan_fetch()
            assert np.array_equal(w, e[5]) and np.array_equal(f, e[6]) and np.array_equal(m, e[7]), a
            ctx.run(channels=4, samples=n)
            _assert_words(ctx.download_f32()[:, :n], e[0], ("the chain's floats", a))
            r = ctx.frames().copy()
            r["sample_pos"] += a // (tr.CH_R1 * tr.CH_D) * tr.CH_U
            recs.append(r)
    finally:
        ctx.close()
    recs = np.concatenate(recs)
    y = np.concatenate([e[0] for e in blocks], axis=1)
    for c in range(4):
        want, got = fl.demod(y[c])[0], recs[recs["channel"] == c]
        assert len(got) == len(want), (c, len(got), len(want))
        for name in ("seq", "cost", "frame_type", "sync_type", "len", "flags", "payload"):
            assert np.array_equal(got[name], want[name]), (c, name)
    assert all(len(tr._good(recs[recs["channel"] == c])) == 7 for c in range(3)) and not (recs["channel"] == 3).any()
