"""CPU-only: the channel meter (ABI 618, include/m17hip.h: m17hip_wide_meter, m17hip_wide_meter_shape, m17hip_wide_meter_fetch).  1: what the new calls
promise without a GPU.  2: the HOST form (detail/core.h's meter_pieces, meter_piece, meter_sum under the host compiler, tests/cxx/meter_oracle.cpp) against
a statement in Python integers and sequential np.float32 adds, bit for bit.  3: windows belong to the feed — however it is cut.  4: what the three sums
mean, against float64 statements with nothing of core.h in them: a carrier of known amplitude and offset, then three transmissions, an empty channel and a
mistuned one in a 2.048 MSPS source."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import meter_lib as ml
import oracle_lib as ol
import resample_lib as rl
import test_resample_input as tr
import wide_lib as wl

U24 = 2.0 ** -24


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1: exports, refusals and the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_meter", "m17hip_wide_meter_shape", "m17hip_wide_meter_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 618
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_meter) and callable(m17hip.Context.wide_meter_fetch)
    assert callable(m17hip.wide_meter_counts) and callable(m17hip.wide_meter_report)
    assert m17hip.KERNELS["meter"] == 16 and m17hip.KERNELS["synth_wide"] == 15 and len(set(m17hip.KERNELS.values())) == len(m17hip.KERNELS)


def test_a_null_context_and_windows_out_of_range_are_refused_and_nothing_is_written():
    lib = m17hip.load_library()
    for window in (0, 1, 15, 16, 1920, 65536, 65537, 0xFFFFFFFF):
        assert lib.m17hip_wide_meter(C.c_void_p(), C.c_uint32(window)) == -1
    c, k, t = C.c_uint32(77), C.c_uint32(78), C.c_uint32(79)
    fw, fo = C.c_uint64(80), C.c_uint64(81)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_meter_shape(C.c_void_p(), C.c_uint32(back), C.byref(c), C.byref(k), C.byref(fw), C.byref(fo), C.byref(t)) == -1
        assert lib.m17hip_wide_meter_shape(C.c_void_p(), C.c_uint32(back), None, None, None, None, None) == -1
    assert (c.value, k.value, t.value, fw.value, fo.value) == (77, 78, 79, 80, 81)
    buf = np.full(64, 7.0, dtype=np.float32)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_meter_fetch(C.c_void_p(), C.c_uint32(back), ol._p(buf), C.c_uint64(64)) == -1
        assert lib.m17hip_wide_meter_fetch(C.c_void_p(), C.c_uint32(back), None, C.c_uint64(64)) == -1
    assert (buf == 7.0).all()


def test_counts_and_report_of_the_python_layer():
    assert m17hip.wide_meter_counts(0, 100, 48).tolist() == [48, 48, 4]
    assert m17hip.wide_meter_counts(47, 100, 48).tolist() == [1, 48, 48, 3]
    assert m17hip.wide_meter_counts((1 << 63) + 5, 3, 48).tolist() == [3]   # ((2^63 + 5) mod 48 = 37)
    assert m17hip.wide_meter_counts((1 << 63) + 5, 12, 48).tolist() == [11, 1]
    for bad in ((0, 0, 48), (0, 5, 0), (-1, 5, 48)):
        with pytest.raises(ValueError):
            m17hip.wide_meter_counts(*bad)
    # a constant y of 0.1 rad at gain 2: 0.05 rad per sample is 48000 * 0.05 / 2 pi Hz, no spread; a power of 100 is 20 dB
    planes = np.array([[[4800.0, 400.0]], [[4.8, 0.4]], [[0.48, 0.04]]])
    r = m17hip.wide_meter_report(planes, [48, 4], 2.0)
    assert np.allclose(r["level_db"], 20.0) and np.allclose(r["offset_hz"], 48000.0 * 0.05 / (2.0 * np.pi))
    assert np.allclose(r["deviation_hz"], 0.0, atol=1e-4)
    # y = +-0.2 at gain 1: mean 0, spread 0.2 rad per sample
    r = m17hip.wide_meter_report(np.array([[[0.0]], [[0.0]], [[48 * 0.04]]]), [48], 1.0)
    assert r["level_db"][0, 0] == -np.inf and r["offset_hz"][0, 0] == 0.0 and np.isclose(r["deviation_hz"][0, 0], 48000.0 * 0.2 / (2.0 * np.pi))
    with pytest.raises(ValueError):
        m17hip.wide_meter_report(np.zeros((3, 2, 2)), [48], 1.0)


# ---- 2: the host form against a statement of its own ---------------------------------------------------------------------------------------------------------
WINDOWS = (16, 17, 48, 1920, 65536)
LENGTHS = (1, 15, 16, 17, 547)
BASES = (0, (1 << 32) + 12345, (1 << 63) + 987654321)


@pytest.mark.parametrize("window", WINDOWS)
def test_pieces_and_sums_are_the_stated_ones_bit_for_bit(window):
    """Every window with every block length, a0 of 0, 1 and window - 1, below 2^32, above it and above 2^63: the pieces are those of Python integers, the
    sums those of sequential np.float32 adds on two levels."""
    rng = np.random.default_rng(6180 + window)
    seen = set()
    for T in LENGTHS:
        for a0 in (0, 1, window - 1):
            for base in BASES:
                N0 = base - base % window + a0
                assert N0 % window == a0 and (base == 0 or N0 >> 32)
                got_a0, K = ml.pieces(N0, T, window)
                stated = ml.pieces_stated(N0, T, window)
                assert (got_a0, K) == (a0, len(stated)) and K == (a0 + T - 1) // window + 1
                assert [ml.piece(a0, T, window, k) for k in range(K)] == stated
                assert m17hip.wide_meter_counts(N0, T, window).tolist() == [m for _, m in stated]
                seen.add(K)
                p = (rng.standard_normal(T) ** 2 * 1e6).astype(np.float32)
                y = rng.uniform(-np.pi, np.pi, T).astype(np.float32)
                got, exp = ml.plane(p, y, N0, window), ml.plane_stated(p, y, N0, window)
                assert got.shape == exp.shape == (3, K) and np.array_equal(_u32(got), _u32(exp)), (T, a0, base)
    assert 1 in seen and (window > 547 and 2 in seen or max(seen) > 2)


def test_the_sum_has_two_levels():
    """1.0 and then 31 values of 2^-24: one chain from +0 never leaves 1.0 (every add is a tie that rounds to even); on two levels the second group of
    sixteen survives as 2^-20.  The order is part of the definition."""
    v = np.array([1.0] + [2.0 ** -24] * 31, dtype=np.float32)
    single = np.float32(0.0)
    for x in v:
        single = np.float32(single + x)
    assert single == np.float32(1.0)
    assert ml.msum(v) == ml.sum_stated(v) == np.float32(1.0 + 2.0 ** -20)
    assert ml.msum(np.zeros(0, dtype=np.float32)) == 0.0
    assert _u32(ml.msum(np.array([-0.0], dtype=np.float32)))[()] == 0   # (chains from +0: +0 + -0 is +0)


# ---- 3: windows belong to the feed -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", (48, 1920))
def test_a_feed_cut_at_multiples_of_the_window_gives_the_uncut_feeds_words(window):
    rng = np.random.default_rng(6190 + window)
    n = 7 * window
    p = (rng.standard_normal(n) ** 2 * 1e6).astype(np.float32)
    y = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    start = (1 << 32) - 2 * window - (1 << 32) % window   # (a multiple of the window; the feed crosses 2^32)
    assert start % window == 0
    whole = ml.plane(p, y, start, window)
    assert whole.shape == (3, 7)
    cuts = [0, window, 3 * window, 4 * window, 7 * window]
    parts = [ml.plane(p[a:b], y[a:b], start + a, window) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(_u32(np.concatenate(parts, axis=1)), _u32(whole))


@pytest.mark.parametrize("window", (48, 1920))
def test_a_ragged_feed_gives_pieces_that_add_up_to_the_windows(window):
    """Blocks of any length: the pieces' counts add up to each window, and in float64 their sums agree with the uncut window's within the bound of the
    chains — a value goes through at most 16 adds on the first level and (groups) on the second, each rounding a partial sum of at most sum|v| by 2^-24 of
    itself (meter_lib.sum_bound): the uncut window's bound plus its pieces'.  A piece boundary off by one output misses it."""
    rng = np.random.default_rng(6200 + window)
    n = 6 * window
    p = (1e6 + rng.standard_normal(n) ** 2 * 1e6).astype(np.float32)
    y = (1.0 + rng.uniform(-0.5, 0.5, n)).astype(np.float32)
    e = (y * y).astype(np.float32)
    whole = ml.plane(p, y, 0, window).astype(np.float64)
    lens = [window // 3, 1, window + 5, 2 * window - 1, window // 2]
    lens.append(n - sum(lens))
    cuts = np.cumsum([0] + lens).tolist()
    assert all(c % window for c in cuts[1:-1])
    for edge in (0, 1, -1):
        acc = np.zeros((3, 6))
        cnt = np.zeros(6, dtype=np.int64)
        bound = np.zeros((3, 6))
        for a, b in zip(cuts[:-1], cuts[1:]):
            pl = ml.plane(p[a:b], y[a:b], a, window, edge=edge)
            for k, (lo, m) in enumerate(ml.pieces_stated(a, b - a, window)):
                wnd = a // window + k
                acc[:, wnd] += pl[:, k]
                cnt[wnd] += m
                for q, v in enumerate((p, y, e)):
                    bound[q, wnd] += ml.sum_bound(v[a + lo:a + lo + m], m)
        assert (cnt == window).all()
        for q, v in enumerate((p, y, e)):
            for wnd in range(6):
                bound[q, wnd] += ml.sum_bound(v[wnd * window:(wnd + 1) * window], window)
        worst = float((np.abs(acc - whole) / bound).max())
        print(f"window {window} edge {edge}: worst |pieces - window| / bound {worst:.3g}")
        if edge == 0:
            assert worst <= 1.0
        else:
            assert worst > 10.0   # (an output in the wrong window: one value of about the mean, against a bound of about 1e-5 of the sum)


# ---- 4: what the sums mean -------------------------------------------------------------------------------------------------------------------------------------
def _report64(p, y, lo, m, gain):
    """level (power, not dB), offset_hz, deviation_hz of outputs lo .. lo + m - 1 in float64 plain sums."""
    p, y = np.asarray(p, dtype=np.float64)[lo:lo + m], np.asarray(y, dtype=np.float64)[lo:lo + m]
    hz = 48000.0 / (2.0 * np.pi * gain)
    return p.mean(), y.mean() * hz, np.sqrt(max((y * y).mean() - y.mean() ** 2, 0.0)) * hz


CARRIER_A, CARRIER_F, CARRIER_GAIN, CARRIER_W = 6000.0, 300.0, 5.0 / 3.0, 48


def test_a_carrier_gives_its_amplitude_and_its_offset_and_no_deviation():
    """An unmodulated carrier of amplitude A, f = 300 Hz above the channel's word, through the one-stage tuner at R = 5 with the default taps.  Once the
    filter is full z[n] = A H(f) e^(j phi n) and y = 2 pi f gain / 48000, so the report is f, A^2 |H(f)|^2 (H from the taps in float64) and 0.  Bounds, as
    wide_lib.f64_bound derives its own: |z - z64| <= bz = f64_bound(sum|h| A, L) + sqrt2 2^-24 A sum|h| (the complex64 samples are the ideal ones rounded);
    p = fma(re, re, im im) is within 2 |z| bz + bz^2 + 2^-23 |z|^2 of |z64|^2; y within dy = gain (2 bz / |z| + 2^-20) (fm_phase's asserted bound);
    e = y y within 2 |y| dy + dy^2 + 2^-24 y^2; a window's mean within the largest of those plus meter_lib.sum_bound / m.  The deviation's bound is the
    square root of the variance's: dy^2 + (bound of mean e) + 2 |y| (bound of mean y).
    Fed the z one output early or late (in the window in which the filter fills, against the float64 statement of that window), or the y without the
    gain, the meter misses them."""
    R, A, f, gain, W = 5, CARRIER_A, CARRIER_F, CARRIER_GAIN, CARRIER_W
    taps = m17hip.wide_default_taps(R)
    L = taps.size
    fcw = m17hip.wide_fcw(30000.0, R)
    n = 10 * W
    m = np.arange(n * R, dtype=np.float64)
    turns = ((m.astype(np.int64) * (fcw & 0xFFFFFFFF)) % (1 << 32)).astype(np.float64) / 4294967296.0 + f / (48000.0 * R) * m
    x = (A * np.exp(2j * np.pi * turns)).astype(np.complex64)
    y, z = wl.Tuner(taps, R, fcw, gain).block(x, want_z=True)
    p = ml.power(z)
    y64, z64, scale = wl.tune_f64(x, taps, R, fcw, gain)
    h = taps.astype(np.float64)
    H = np.sum(h * np.exp(-2j * np.pi * f / (48000.0 * R) * np.arange(L)))
    level, y0 = A * A * abs(H) ** 2, 2.0 * np.pi * f * gain / 48000.0
    bz = wl.f64_bound(scale, L) + np.sqrt(2.0) * U24 * A * np.abs(h).sum()
    hz = 48000.0 / (2.0 * np.pi * gain)
    counts = m17hip.wide_meter_counts(0, n, W)
    rep = m17hip.wide_meter_report(ml.plane(p, y, 0, W)[:, None, :], counts, gain)
    first_full = -(-(-(-L // R) + 1) // W)   # the first window all of whose outputs (and the z in front of them) have a full filter
    assert first_full == 1 and n // W >= 5
    worst = {}
    for k in range(first_full, n // W):
        lo = k * W
        mag = abs(z64[lo:lo + W]).min()
        assert mag > 0.99 * A * abs(H)
        dy = gain * (2.0 * bz / mag + 2.0 ** -20)
        b_level = 2.0 * np.sqrt(level) * bz + bz * bz + 2.0 * U24 * level + ml.sum_bound(p[lo:lo + W], W) / W
        b_mean = dy + ml.sum_bound(y[lo:lo + W], W) / W
        b_e = 2.0 * y0 * dy + dy * dy + U24 * y0 * y0 + ml.sum_bound(y[lo:lo + W] ** 2, W) / W
        b_dev = np.sqrt(dy * dy + b_e + 2.0 * y0 * b_mean + b_mean ** 2) * hz
        got = (10.0 ** (rep["level_db"][0, k] / 10.0), rep["offset_hz"][0, k], rep["deviation_hz"][0, k])
        for name, g, want, b in (("level", got[0], level, b_level), ("offset", got[1], f, b_mean * hz), ("deviation", got[2], 0.0, b_dev)):
            worst[name] = max(worst.get(name, 0.0), abs(g - want) / b)
        # the y without the gain: the offset is f / gain
        bad = m17hip.wide_meter_report(ml.plane(p, y / np.float32(gain), 0, W)[:, None, :], counts, gain)
        assert abs(bad["offset_hz"][0, k] - f) > 100.0 * b_mean * hz
    print("carrier: worst error over its bound", {k: round(v, 4) for k, v in worst.items()}, f"bounds: level {b_level / level:.2e} of it, "
          f"offset {b_mean * hz:.3f} Hz, deviation {b_dev:.3f} Hz")
    assert max(worst.values()) <= 1.0
    # window 0, in which the filter fills: the level against the float64 statement of the same outputs; z one output early or late misses it
    p64 = np.abs(z64[:W]) ** 2
    b0 = float(np.mean(2.0 * np.abs(z64[:W]) * bz + bz * bz + 2.0 * U24 * p64)) + ml.sum_bound(p[:W], W) / W
    assert abs(10.0 ** (rep["level_db"][0, 0] / 10.0) - p64.mean()) <= b0
    for shifted in (np.concatenate([[np.float32(0.0)], p[:-1]]), np.concatenate([p[1:], p[-1:]])):
        bad = m17hip.wide_meter_report(ml.plane(shifted, y, 0, W)[:, None, :], counts, gain)
        assert abs(10.0 ** (bad["level_db"][0, 0] / 10.0) - p64.mean()) > 100.0 * b0


EMPTY_HZ, LOW_HZ, SRC_W = 400000.0, 300.0, 1920
# MEASURED on the host form over the six frame windows (this test prints them; NOTES.md has them):
#   levels 75.45, 75.45, 75.45 dB on the three transmissions, 75.44 dB on the mistuned channel, 38.59 dB on the empty one: 36.45 dB at the least;
#   deviations 1844, 1850, 1850 and 1848 Hz (the RMS of M17's four levels, +-2400 and +-800 Hz, is 1789 Hz) against 4552 Hz of discriminator noise: a ratio
#   of 2.029 at the least;
#   offsets 36, 12 and 12 Hz on the tuned channels — the mean of six frames' symbols is not zero: single windows read up to 75 Hz off — and 312 Hz on the
#   channel tuned 300 Hz low: within 74.99 Hz of 300 by itself, within 0.116 Hz against the well-tuned channel on the same transmission.
MEASURED_LEVEL_DB = 36.45
MEASURED_DEV_RATIO = 2.029
MEASURED_OFFSET_ERR_HZ = 74.99
MEASURED_OFFSET_REL_ERR_HZ = 0.116


def test_three_transmissions_an_empty_channel_and_a_mistuned_one():
    """tests/test_resample_input.py's 2.048 MSPS source: channels on its three transmissions, one on an empty stretch of the band (+400 kHz) and one tuned
    300 Hz below the second transmission, through the resampling tuner's host form at one window per M17 frame (1920 outputs), over the windows the
    transmissions fill.  Against the float64 statement (resample_lib.resample_f64: its |z|^2 and y in plain float64 sums) the host form's level is within
    the carrier test's bound; the offset and the deviation are checked where that statement's y means something (|z| above 8 bounds on every output of the
    window — an empty channel's z passes through zero, where no bound on a phase holds).  Then what a user reads off: how far the carried channels' level
    stands over the empty one's, how much wider the empty channel's discriminator noise is than a transmission's deviation, and the 300 Hz."""
    R1, U, D = tr.CH_R1, tr.CH_U, tr.CH_D
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tr.KINDS]
    x = tr.source_2048k(bb)
    taps1, taps2 = m17hip.wide_resample_default_taps(R1, U, D)
    hz = [tr.OFFSETS[0], tr.OFFSETS[1], tr.OFFSETS[2], EMPTY_HZ, tr.OFFSETS[1] - LOW_HZ]
    n = x.shape[0] // (R1 * D) * U
    windows = range(9600 // SRC_W, (9600 + 6 * 1920) // SRC_W)   # the windows every transmission fills with frames
    rep, rep64 = [], []
    for c, f in enumerate(hz):
        fcw = m17hip.wide_fcw(f, R1 * D / U)
        y, z = rl.Resampler(taps1, R1, U, D, taps2, fcw, 1.0).block(x, want_z=True)
        p = ml.power(z)
        counts = m17hip.wide_meter_counts(0, n, SRC_W)
        r = m17hip.wide_meter_report(ml.plane(p, y, 0, SRC_W)[:, None, :], counts, 1.0)
        y64, z64, scale = rl.resample_f64(x, taps1, R1, U, D, taps2, fcw, 1.0)
        bz = rl.f64_bound(scale, taps1.size, taps2.size, U)
        rows = []
        for k in windows:
            lo = k * SRC_W
            p64 = np.abs(z64[lo:lo + SRC_W]) ** 2
            lvl64, off64, dev64 = _report64(p64, y64, 0, SRC_W, 1.0)[0], *_report64(p64, y64[lo:lo + SRC_W], 0, SRC_W, 1.0)[1:]
            lvl = 10.0 ** (r["level_db"][0, k] / 10.0)
            b_level = float(np.mean(2.0 * np.abs(z64[lo:lo + SRC_W]) * bz + bz * bz + 2.0 * U24 * p64)) + ml.sum_bound(p[lo:lo + SRC_W], SRC_W) / SRC_W
            assert abs(lvl - lvl64) <= b_level, (c, k)
            mag = np.minimum(np.abs(z64[lo:lo + SRC_W]), np.abs(z64[lo - 1:lo + SRC_W - 1])).min()
            if mag > 8.0 * bz and np.abs(y64[lo:lo + SRC_W]).max() < 3.0:   # (no output near the wrap either)
                dy = 2.0 * bz / mag + 2.0 ** -20
                ymax = float(np.abs(y64[lo:lo + SRC_W]).max())
                b_mean = dy + ml.sum_bound(y[lo:lo + SRC_W], SRC_W) / SRC_W
                b_e = 2.0 * ymax * dy + dy * dy + U24 * ymax ** 2 + ml.sum_bound(y[lo:lo + SRC_W] ** 2, SRC_W) / SRC_W
                b_var = b_e + 2.0 * ymax * b_mean + b_mean ** 2
                k_hz = 48000.0 / (2.0 * np.pi)
                assert abs(r["offset_hz"][0, k] - off64) <= b_mean * k_hz, (c, k)
                assert abs((r["deviation_hz"][0, k] / k_hz) ** 2 - (dev64 / k_hz) ** 2) <= b_var, (c, k)
                rows.append(k)
        assert (len(rows) == len(windows)) == (c != 3), (c, rows)   # (every window of a carried channel; the empty channel is not spoken about)
        rep.append({q: r[q][0, list(windows)] for q in r})
    level = np.array([r["level_db"] for r in rep])
    dev = np.array([r["deviation_hz"] for r in rep])
    off = np.array([r["offset_hz"] for r in rep])
    sep_db = float((level[[0, 1, 2, 4]] - level[3]).min())
    dev_ratio = float((dev[3] / dev[[0, 1, 2, 4]]).min())
    off_err = float(np.abs(off[4] - LOW_HZ).max())              # the mistuned channel's own reading
    rel_err = float(np.abs((off[4] - off[1]) - LOW_HZ).max())   # against the well-tuned channel on the same transmission
    print(f"measured: carried over empty {sep_db:.2f} dB at the least (levels {np.round(level.mean(axis=1), 2).tolist()} dB), empty / carried deviation "
          f"{dev_ratio:.3f} at the least (deviations {np.round(dev.mean(axis=1), 1).tolist()} Hz), the 300 Hz within {off_err:.3f} Hz ({rel_err:.3f} Hz against the tuned channel) "
          f"(offsets {np.round(off.mean(axis=1), 2).tolist()} Hz)")
    # half the measured separation as margin for the two ratios (in dB; as a ratio over 1), twice the measured error for the offset
    assert sep_db >= 0.5 * MEASURED_LEVEL_DB
    assert dev_ratio >= 1.0 + 0.5 * (MEASURED_DEV_RATIO - 1.0)
    assert off_err <= 2.0 * MEASURED_OFFSET_ERR_HZ and rel_err <= 2.0 * MEASURED_OFFSET_REL_ERR_HZ
