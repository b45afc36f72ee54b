"""CPU-only: the spectrum squelch (ABI 619, include/m17hip.h: m17hip_wide_squelch, m17hip_wide_squelch_fetch).  1: what the new calls promise without a GPU.
2: the HOST form (detail/core.h's squelch_bin, squelch_band, squelch_level, squelch_step under the host compiler, tests/cxx/squelch_oracle.cpp) against a
statement in Python integers and sequential np.float32 adds, bit for bit.  3: the step on crafted sequences.  4: what it means, on the 2.048 MSPS source of
three transmissions of tests/test_resample_input.py with channels on empty spectrum beside them, and the sign convention of a channel's bin."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_lib as sq
import test_resample_input as tr
import wide_lib as wl

OPEN = sq.OPEN


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1: exports, refusals and the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_squelch", "m17hip_wide_squelch_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 619
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_squelch) and callable(m17hip.Context.wide_squelch_fetch)
    assert callable(m17hip.wide_squelch_half_bins) and callable(m17hip.wide_squelch_levels)
    assert m17hip.KERNELS["squelch"] == 17 and m17hip.KERNELS["meter"] == 16 and len(set(m17hip.KERNELS.values())) == len(m17hip.KERNELS)


def test_a_null_context_and_arguments_out_of_range_are_refused_and_nothing_is_written():
    lib = m17hip.load_library()
    lv = np.array([2.0, 1.0], dtype=np.float32)
    for half, n, hang in ((0, 0, 0), (4, 1, 0), (65, 1, 0), (4, 1, 65536), (0xFFFFFFFF, 1, 0xFFFFFFFF)):
        assert lib.m17hip_wide_squelch(C.c_void_p(), C.c_uint32(half), ol._p(lv) if n else None, ol._p(lv[1:]) if n else None, C.c_uint32(n),
                                       C.c_uint32(hang)) == -1
    state, band = np.full(8, 77, dtype=np.uint32), np.full(8, 7.0, dtype=np.float32)
    n, frames = C.c_uint32(78), C.c_uint32(79)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_squelch_fetch(C.c_void_p(), C.c_uint32(back), ol._p(state), ol._p(band), C.c_uint64(8), C.byref(n), C.byref(frames)) == -1
        assert lib.m17hip_wide_squelch_fetch(C.c_void_p(), C.c_uint32(back), None, None, C.c_uint64(8), None, None) == -1
    assert (state == 77).all() and (band == 7.0).all() and (n.value, frames.value) == (78, 79)


def test_half_bins_and_levels_of_the_python_layer():
    assert m17hip.wide_squelch_half_bins(9000.0, 2048000.0, 2048) == 4     # (4.5 bins of 1 kHz: Python rounds the tie to even, as wide_spectrum_carriers does)
    assert m17hip.wide_squelch_half_bins(9000.0, 240000.0, 64) == 1        # (1.2 bins of 3.75 kHz)
    assert m17hip.wide_squelch_half_bins(1.0e9, 240000.0, 64) == 31        # (never the whole circle)
    assert m17hip.wide_squelch_half_bins(100.0, 2048000.0, 64) == 0
    assert m17hip.wide_squelch_half_bins(9000.0, 240000.0, 4096) == 64     # (77 bins of 58.6 Hz: m17hip_wide_squelch takes 64 at the most)
    # two sources whose floors are 3 and 50 per bin over 10 frames; one strong bin does not move a median
    p = np.array([[30.0] * 63 + [1.0e9], [500.0] * 64])
    o, c = m17hip.wide_squelch_levels(p, 10, 2, 10.0, 3.0)
    assert o.dtype == np.float32 and c.dtype == np.float32 and o.shape == (2,)
    assert np.allclose(o, [3.0 * 5 * 10.0, 50.0 * 5 * 10.0], rtol=1e-6) and np.allclose(c, np.array([15.0, 250.0]) * 10.0 ** 0.3, rtol=1e-6)
    assert (c <= o).all()
    with pytest.raises(ValueError):
        m17hip.wide_squelch_levels(p, 0, 2, 10.0, 3.0)


# ---- 2: the host form against a statement of its own ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", range(6, 13))
def test_the_bin_of_a_word(logn):
    """Every N in 64..4096: the extreme words, 0 and -1, and every rounding edge +-2^(31 - log2 N) - {0, 1} of bins 0, 1, N / 2 - 1, N / 2 and N - 1."""
    N, half, width = 1 << logn, 1 << (31 - logn), 1 << (32 - logn)
    words = [-(1 << 31), (1 << 31) - 1, 0, -1]
    for k in (0, 1, N // 2 - 1, N // 2, N - 1):
        centre = k * width if k < N // 2 else (k - N) * width
        for edge in (half, -half):
            for d in (0, 1):
                w = centre + edge - d
                if -(1 << 31) <= w < (1 << 31):
                    words.append(w)
    for w in words:
        assert sq.bin_(w, logn) == sq.bin_stated(w, logn), (logn, w)
    # what the rule means: the word of bin k's own frequency gives k, a word half a bin up rounds up, one less stays; the top half bin wraps to N / 2
    assert sq.bin_(0, logn) == 0 and sq.bin_(-1, logn) == 0 and sq.bin_(width, logn) == 1 and sq.bin_(-width, logn) == N - 1
    assert sq.bin_(half, logn) == 1 and sq.bin_(half - 1, logn) == 0 and sq.bin_(-half, logn) == 0 and sq.bin_(-half - 1, logn) == N - 1
    assert sq.bin_(-(1 << 31), logn) == N // 2 and sq.bin_((1 << 31) - 1, logn) == N // 2 and sq.bin_((1 << 31) - half - 1, logn) == N // 2 - 1


@pytest.mark.parametrize("N", (64, 2048))
def test_the_band_is_a_circular_chain_in_a_fixed_order(N):
    rng = np.random.default_rng(6190 + N)
    row = (rng.standard_normal(N) ** 2 * 10.0 ** rng.uniform(-3, 9, N)).astype(np.float32)
    special = row.copy()
    special[[3, N - 2]] = np.inf
    special[[7, N // 2]] = np.nan
    special[[N - 1]] = 0.0
    for r in (row, special):
        for B in (0, 1, min(64, N // 2 - 1)):
            for k in (0, 1, 2, 3, 7, N // 2, N - 3, N - 2, N - 1):
                got, exp = sq.band(r, k, B), sq.band_stated(r, k, B)
                assert _u32(got) == _u32(exp) or (np.isnan(got) and np.isnan(exp)), (N, B, k)
    # the order is part of the definition: d ascending from -B, across the wrap.  1 + 1 + 2^24 is 2^24 + 2; begun at the other end it is 2^24
    r = np.zeros(N, dtype=np.float32)
    r[[N - 1, 0, 1]] = [1.0, 1.0, 2.0 ** 24]
    assert sq.band(r, 0, 1) == np.float32(2.0 ** 24 + 2.0) and np.float32(np.float32(r[1] + r[0]) + r[N - 1]) == np.float32(2.0 ** 24)


def test_a_level_is_one_rounded_multiply():
    for lv, J in ((np.float32(1.1), 3), (np.float32(3.3333333e7), 500), (np.float32(1.0e-30), 7), (np.float32(1.0), 0)):
        assert _u32(sq.level(lv, J)) == _u32(np.float32(lv * np.float32(J)))


# ---- 3: the step -----------------------------------------------------------------------------------------------------------------------------------------------
def _run(bands, hang, to=10.0, tc=5.0, h=0, J=4):
    out = []
    for b in bands:
        w = sq.step(h, b, to, tc, hang, J)
        assert w == sq.step_stated(h, b, to, tc, hang, J), (h, b, hang)
        h = w & ~OPEN
        out.append((bool(w & OPEN), h))
    return out


def test_the_step_on_crafted_sequences():
    T, F = True, False
    # opening at the level itself (the comparison is !(b < to)), and not a hair below
    assert _run([9.999999, 10.0, 11.0], 0) == [(F, 0), (T, 1), (T, 1)]
    # between close and open: closed stays closed; open is re-armed
    assert _run([7.0, 7.0], 2) == [(F, 0), (F, 0)]
    assert _run([12.0, 7.0, 7.0, 5.0, 4.999], 2) == [(T, 3), (T, 3), (T, 3), (T, 3), (T, 2)]
    # the countdown at hang 0, 1, 3
    assert _run([12.0, 1.0, 1.0], 0) == [(T, 1), (F, 0), (F, 0)]
    assert _run([12.0, 1.0, 1.0, 1.0], 1) == [(T, 2), (T, 1), (F, 0), (F, 0)]
    assert _run([12.0, 1.0, 1.0, 1.0, 1.0, 1.0], 3) == [(T, 4), (T, 3), (T, 2), (T, 1), (F, 0), (F, 0)]
    # re-armed in the middle of a countdown by a band over the close level
    assert _run([12.0, 1.0, 6.0, 1.0], 3) == [(T, 4), (T, 3), (T, 4), (T, 3)]
    # a block without a frame: open, the count as it was — closed before and after, or still counting
    assert _run([0.0], 2, J=0) == [(T, 0)] and _run([0.0], 2, h=2, J=0) == [(T, 2)]
    assert sq.step(0, 1.0, 10.0, 5.0, 2, 0) == OPEN and sq.step(0, 1.0, 10.0, 5.0, 2, 1) == 0
    # a NaN band opens, and holds open
    assert _run([np.nan], 1) == [(T, 2)] and _run([np.nan], 0, h=1) == [(T, 1)]
    # the largest hang
    assert sq.step(0, 11.0, 10.0, 5.0, 65535, 1) == (65536 | OPEN)


def test_a_block_of_decisions_is_the_steps_of_its_channels():
    rng = np.random.default_rng(6191)
    plane = (rng.standard_normal((2, 64)) ** 2 * 100.0).astype(np.float32)
    src, fcw = [0, 1, 1, 0], [0, -(1 << 31), (1 << 31) - 1, 12345 << 12]
    o, c = np.array([300.0, 250.0], dtype=np.float32), np.array([200.0, 250.0], dtype=np.float32)
    s = sq.Squelch(src, fcw, o, c, 1, 2)
    s.hold[:] = [0, 1, 2, 3]
    hold = s.hold.copy()
    state, band = s.block(plane, 3)
    for ch in range(4):
        b = sq.band_stated(plane[src[ch]], sq.bin_stated(fcw[ch], 6), 1)
        assert _u32(band[ch]) == _u32(b)
        assert int(state[ch]) == sq.step_stated(int(hold[ch]), b, np.float32(o[src[ch]] * np.float32(3)), np.float32(c[src[ch]] * np.float32(3)), 2, 3)
        assert int(s.hold[ch]) == int(state[ch]) & ~OPEN


# ---- 4: meaning ------------------------------------------------------------------------------------------------------------------------------------------------
POINTS, HOP = 2048, 2048
OPEN_DB, CLOSE_DB, HANG = 10.0, 6.0, 1
EMPTY = (400000.0, -300000.0, 900000.0, 62500.0)   # Hz: nobody transmits there (the last is 37.5 kHz from the nearest carrier)
BLOCK = 4800                                        # outputs per block: 100 ms, 204 800 source samples, 100 frames


@functools.lru_cache(maxsize=None)
def _source():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tr.KINDS]
    x = tr.source_2048k(bb)
    x.setflags(write=False)
    return bb, x


def _squelched_feed(block, open_db=OPEN_DB, close_db=CLOSE_DB, hang=HANG):
    """The host-form resampler over the source in blocks of `block` outputs, squelched at levels taken from the first block's plane: per channel the floats,
    and per block the open flags."""
    bb, x = _source()
    rate = 2048000.0
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    offs = list(tr.OFFSETS) + list(EMPTY)
    fcw = [m17hip.wide_fcw(f, tr.CH_R1 * tr.CH_D / tr.CH_U) for f in offs]
    B = m17hip.wide_squelch_half_bins(9000.0, rate, POINTS)
    step = block // tr.CH_U * tr.CH_R1 * tr.CH_D
    p0, J0, _ = spl.plane(x[:step], POINTS, HOP)
    o, c = m17hip.wide_squelch_levels(p0[None, :], J0, B, open_db, close_db)
    feed = sq.Feed([rl.Resampler(taps1, tr.CH_R1, tr.CH_U, tr.CH_D, taps2, w) for w in fcw], [0] * len(fcw), [x], POINTS, HOP)
    feed.squelch = sq.Squelch([0] * len(fcw), fcw, o, c, B, hang)
    ys, opens, frames = [], [], []
    for a in range(0, x.shape[0], step):
        Y, P, state, band, J = feed.block(a, min(a + step, x.shape[0]))
        ys.append(Y)
        opens.append((state & OPEN) != 0)
        frames.append(J)
    return np.concatenate(ys, axis=1), np.array(opens), frames


def test_transmissions_stay_open_and_empty_channels_closed_and_the_frames_are_kept():
    """Blocks of 100 ms, a band of 9 kHz, open 10 dB and close 6 dB over the median floor, hang 1.  The three carriers are there from the source's first
    sample to its last (the generator's lead-in and tail are carrier too), so their channels are open in every block; the four channels on empty spectrum
    are closed in every block that holds a frame, and their floats are +0; the float oracle decodes from the squelched floats what it decodes from the
    unsquelched feed."""
    bb, x = _source()
    y, opens, frames = _squelched_feed(BLOCK)
    assert all(J > 0 for J in frames[:-1])
    have = np.array(frames) > 0
    assert opens[:, :3].all(), opens[:, :3]
    assert not opens[have][:, 3:].any(), opens[:, 3:]
    n_have = int(have.sum()) * BLOCK if have.all() else int(np.argmin(have)) * BLOCK
    assert (_u32(y[3:, :n_have]) == 0).all()
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    for c, (s, f) in enumerate(zip(bb, tr.OFFSETS)):
        plain = rl.resample(x, taps1, tr.CH_R1, tr.CH_U, tr.CH_D, taps2, m17hip.wide_fcw(f, tr.CH_R1 * tr.CH_D / tr.CH_U))
        assert np.array_equal(_u32(plain), _u32(y[c])), f   # (never closed: the very words)
        got, exp = fl.demod(y[c])[0], fl.demod(plain)[0]
        assert np.array_equal(got, exp) and len(tr._good(got)) == 7, f


def test_a_tone_opens_the_channel_at_its_own_word_and_not_at_the_mirrored_one():
    """A tone at +f is exp(+2 pi i f n / Fs): bin f N / Fs of the spectrum.  wide_fcw(+f) opens; wide_fcw(-f) looks at bin N - f N / Fs and stays closed."""
    rate, f, N = 240000.0, 45000.0, 256
    n = np.arange(16 * N)
    rng = np.random.default_rng(6192)
    x = 6000.0 * np.exp(2j * np.pi * f * n / rate) + 30.0 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    row = np.clip(np.rint(np.stack([x.real, x.imag], axis=-1)), -32768, 32767).astype(np.int16)
    plane, J, _ = spl.plane(row, N, N)
    assert J == 16 and int(np.argmax(plane)) == int(round(f * N / rate))
    B = m17hip.wide_squelch_half_bins(9000.0, rate, N)
    o, c = m17hip.wide_squelch_levels(plane[None, :], J, B, 10.0, 6.0)
    s = sq.Squelch([0, 0], [m17hip.wide_fcw(f, 5), m17hip.wide_fcw(-f, 5)], o, c, B, 0)
    state, band = s.block(plane[None, :], J)
    assert (state & OPEN).astype(bool).tolist() == [True, False], (state, band, o)
    assert band[0] > 1000.0 * band[1]
