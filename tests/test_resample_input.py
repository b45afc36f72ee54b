"""CPU-only: wideband IQ input at rational sample rates (ABI 615, include/m17hip.h: m17hip_wide_resample, m17hip_wide_resample_default_taps,
m17hip_wide_resample_ratio).  1: at up = 1 the HOST form (detail/core.h's ddc_resample under the host compiler, tests/cxx/resample_oracle.cpp) gives the
two-stage tuner's words.  2: the whole operation against a plain float64 statement of it — zero-stuffing, np.convolve, the sample at n D + D - 1 —, within a
derived bound which a wrong tap phase or a wrong kept sample misses.  3: the default taps.  4: the ratio a rate has.  5: a feed cut into blocks gives the
words of the uncut feed.  6: the feature means something — three FM transmissions in one 2.048 MSPS source carry their basebands' frames.  7: what the new
calls promise without a GPU."""
import ctypes as C
import os
import shutil
import subprocess
from math import gcd

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import resample_lib as rl
import wide2_lib as w2
import wide_lib as wl

LICH = 1


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _taps(rng, L):
    return (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)


# ---- 1: up = 1 is the two-stage tuner --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 3, 5, 7), (10, 5, 81, 161), (16, 1, 129, 33)], ids=lambda c: "{}x{}_{}_{}".format(*c))
def test_up_1_gives_the_two_stage_tuners_words(case):
    R1, D, L1, L2 = case
    rng = np.random.default_rng(6150 + D)
    cuts = np.cumsum([0, 1, 2, 85, 1, 100, 3, 67]).tolist()
    x = rng.integers(-20000, 20001, size=(cuts[-1] * R1 * D, 2)).astype(np.int16)
    taps1, taps2 = _taps(rng, L1), _taps(rng, L2)
    fcw = m17hip.wide_fcw(31000.0, R1 * D)
    whole = w2.tune2(x, taps1, R1, taps2, D, fcw, 1.25)
    assert np.array_equal(_u32(rl.resample(x, taps1, R1, 1, D, taps2, fcw, 1.25)), _u32(whole))
    t = rl.Resampler(taps1, R1, 1, D, taps2, fcw, 1.25)
    parts = [t.block(x[a * R1 * D: b * R1 * D]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(_u32(np.concatenate(parts)), _u32(whole))
    assert rl.hist_len(L1, R1, L2, 1) == w2.hist_len(L1, R1, L2)


# ---- 2: against float64 ----------------------------------------------------------------------------------------------------------------------------------
# rl.resample_f64 on wide_lib.carriers, the default taps.  1200 outputs: the default channel filter spans 32 outputs, and the first of a feed — a fixed
# number of them, not a share — are partial sums of its side lobes, below the magnitude the y rule needs (wide_lib.hamming_taps' docstring).
# The bounds are DERIVED as wide2_lib.f64_bound2's are, with the taps a z actually meets:
#   |z_host - z_f64| <= scale (2^-20.5 + (L1 + ceil(L2 / U) + 2) 2^-24), scale = max_r sum|taps2[r::U]| sum|taps1| max|x|;
#   |y_host - y_f64| (mod 2 pi) <= gain (2 bound / min|z| + 2^-20) wherever z[n] and z[n-1] of the reference both exceed 8 bound (wide_lib.f64_check_y's rule).
# At most 1 % of a case's outputs may fall under that floor (tests/test_wide2_input.py's cap): asserted on the float64 reference alone.
F64_CASES = [(8, 3, 16), (5, 12, 125), (5, 2, 25), (1, 24, 125)]   # (decim1, up, down)
# (decim1, up, down, ntaps1, ntaps2) of tests/test_gpu_resample_tiles.py: every class with exactly 8 taps, and 32 classes of 8 or 9 taps behind a stage 1 that
# does nothing.  Hamming windows (wide_lib.hamming_taps: the carrier is mixed to 0 Hz, inside any low-pass), the second one times `up` so that every branch has
# a DC gain near 1
F64_TAPPED = [(2, 3, 4, 9, 24), (1, 32, 33, 1, 265)]
F64_N = 1200
F64_GAIN = 1.25
F64_WORDS = {"generic": -0x12345679, "+2^30": 1 << 30}
F64_EXCLUDED_CAP = 0.01


def _f64_taps(case):
    if len(case) == 3:
        return m17hip.wide_resample_default_taps(*case)
    R1, U, D, L1, L2 = case
    return wl.hamming_taps(L1), (U * wl.hamming_taps(L2).astype(np.float64)).astype(np.float32)


def _f64_input(case, fcw, fmt=wl.IQ_I16):
    R1, U, D = case[:3]
    n = -(-F64_N // U) * U
    return wl.carriers(R1 * D, [fcw], n // U, fmt, seed=6151 + D), n


@pytest.mark.parametrize("case", F64_CASES + F64_TAPPED, ids=lambda c: "{}_{}over{}".format(*c) + ("_{}_{}".format(*c[3:]) if len(c) > 3 else ""))
def test_the_resampler_is_within_derived_bounds_of_float64(case):
    R1, U, D = case[:3]
    taps1, taps2 = _f64_taps(case)
    assert len(case) == 3 or (taps1.size, taps2.size) == case[3:]
    worst = [0.0, 0.0, 0.0]
    for name, fcw in F64_WORDS.items():
        x, n = _f64_input(case, fcw)
        y64, z64, scale = rl.resample_f64(x, taps1, R1, U, D, taps2, fcw, F64_GAIN)
        assert z64.size == n
        bound = rl.f64_bound(scale, taps1.size, taps2.size, U)
        excluded = 1.0 - float(w2.f64_ok(z64, bound).mean())
        assert excluded <= F64_EXCLUDED_CAP, (case, name, excluded)
        y, z = rl.Resampler(taps1, R1, U, D, taps2, fcw, F64_GAIN).block(x, want_z=True)
        ez, ey, _ = w2.f64_errors(y, z, y64, z64, bound, F64_GAIN)
        assert y[0] == 0.0 and y64[0] == 0.0
        print(f"resampler vs float64, {case} {name}: z error {ez:.3f} of its bound, y error {ey:.3f}, excluded {100 * excluded:.2f} %")
        assert ez <= 1.0 and ey <= 1.0, (case, name, ez, ey)
        worst = [max(a, b) for a, b in zip(worst, (ez, ey, excluded))]


@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: "{}_{}over{}".format(*c))
def test_a_wrong_tap_phase_or_kept_sample_misses_the_z_bound(case):
    """The float64 statement with the taps i0 + 1 + U j in place of i0 + U j, or with sample n D + D - 2 of the stuffed and filtered feed kept: the host form
    is far outside the bound it meets against the right one."""
    R1, U, D = case
    taps1, taps2 = m17hip.wide_resample_default_taps(R1, U, D)
    fcw = F64_WORDS["generic"]
    x, _ = _f64_input(case, fcw)
    _, z = rl.Resampler(taps1, R1, U, D, taps2, fcw, F64_GAIN).block(x, want_z=True)
    _, right, scale = rl.resample_f64(x, taps1, R1, U, D, taps2, fcw, F64_GAIN)
    _, phase, _ = rl.resample_f64(x, taps1, R1, U, D, taps2, fcw, F64_GAIN, phase=1)
    _, kept, _ = rl.resample_f64(x, taps1, R1, U, D, taps2, fcw, F64_GAIN, keep=D - 2)
    bound = rl.f64_bound(scale, taps1.size, taps2.size, U)
    e = [float(np.abs(z - r).max()) / bound for r in (right, phase, kept)]
    print(f"{case}: z error over its bound: right {e[0]:.3f}, phase i0 + 1 {e[1]:.1f}, sample n D + D - 2 kept {e[2]:.1f}")
    assert e[0] <= 1.0
    assert e[1] > 10.0 and e[2] > 10.0


# ---- 3: the default taps ---------------------------------------------------------------------------------------------------------------------------------
def _sinc64(L, fc, gain=1.0):
    i = np.arange(L, dtype=np.float64)
    t = i - 0.5 * (L - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 2.0 * fc, np.sin(2.0 * np.pi * fc * t) / (np.pi * t))
    h = s * (0.42 - 0.5 * np.cos(2.0 * np.pi * i / (L - 1)) + 0.08 * np.cos(4.0 * np.pi * i / (L - 1)))
    return h / h.sum() * gain


TAP_PAIRS = [(16, 3), (125, 12), (25, 2), (125, 3), (20, 3), (15, 2), (3, 2), (125, 24)]   # (down, up)


@pytest.mark.parametrize("D,U", TAP_PAIRS)
def test_default_taps_follow_their_formulas(D, U):
    for R1 in (1, 5, 16):
        taps1, taps2 = m17hip.wide_resample_default_taps(R1, U, D)
        assert taps1.dtype == np.float32 and taps2.dtype == np.float32 and taps2.size == 32 * D + 1
        if R1 == 1:
            assert taps1.tolist() == [1.0]
        else:
            assert taps1.size == 8 * R1 + 1
            assert np.abs(taps1.astype(np.float64) - _sinc64(8 * R1 + 1, 0.5 / R1)).max() <= 2.0 ** -24   # (a rounding of a tap below 1 / 2, and libm's last bit)
    e = _sinc64(32 * D + 1, 5500.0 / (48000.0 * D), float(U))
    assert np.abs(taps2.astype(np.float64) - e).max() <= 2.0 ** -24 * max(1.0, np.abs(e).max())
    # every branch of the polyphase filter has unit DC gain: in float64 the formula is within 9.0e-8 for these pairs, the rounding adds about 4e-8
    branch = [abs(float(taps2[r::U].astype(np.float64).sum()) - 1.0) for r in range(U)]
    print(f"down {D}, up {U}: branch sums within {max(branch):.2e} of 1")
    assert max(branch) <= 1e-6


def test_default_taps_at_up_1_are_the_raster_defaults():
    for D in (1, 5, 16, 25, 64):
        for R1 in (1, 10):
            taps1, taps2 = m17hip.wide_resample_default_taps(R1, 1, D)
            assert np.array_equal(_u32(taps2), _u32(m17hip.wide_raster_default_taps(D)))
            if D <= 16:
                e1, e2 = m17hip.wide_default_taps2(R1, D)
                assert np.array_equal(_u32(taps2), _u32(e2)) and taps1.size == e1.size


def _defaults(d1, up, down, t1, c1, n1, t2, c2, n2):
    return m17hip.load_library().m17hip_wide_resample_default_taps(C.c_uint32(d1), C.c_uint32(up), C.c_uint32(down), t1, C.c_uint32(c1), n1, t2,
                                                                   C.c_uint32(c2), n2)


def test_default_taps_refusals():
    n1, n2 = C.c_uint32(0), C.c_uint32(0)
    b1, b2 = np.full(200, 7.0, dtype=np.float32), np.full(4100, 7.0, dtype=np.float32)
    p1, p2 = ol._p(b1), ol._p(b2)
    for d1, up, down in ((0, 3, 8), (17, 3, 8), (16, 0, 8), (16, 33, 125), (16, 3, 0), (16, 3, 126), (16, 9, 8), (16, 6, 8), (16, 2, 2)):
        assert _defaults(d1, up, down, p1, 200, C.byref(n1), p2, 4100, C.byref(n2)) == -1, (d1, up, down)
    for d1, up, down in ((1, 1, 1), (16, 32, 125), (1, 1, 125), (16, 31, 32)):   # (the limits themselves are served)
        assert _defaults(d1, up, down, p1, 200, C.byref(n1), p2, 4100, C.byref(n2)) == 0, (d1, up, down)
        assert (n1.value, n2.value) == (1 if d1 == 1 else 8 * d1 + 1, 32 * down + 1)
    b1[:], b2[:] = 7.0, 7.0
    assert _defaults(16, 3, 8, p1, 128, C.byref(n1), p2, 4100, C.byref(n2)) == -1 and (n1.value, n2.value) == (129, 257)   # (too small: the lengths are still said)
    assert _defaults(16, 3, 8, p1, 200, C.byref(n1), p2, 256, C.byref(n2)) == -1 and (n1.value, n2.value) == (129, 257)
    assert _defaults(16, 3, 8, None, 200, C.byref(n1), p2, 4100, C.byref(n2)) == -1
    assert _defaults(16, 3, 8, p1, 200, C.byref(n1), None, 4100, C.byref(n2)) == -1
    assert _defaults(16, 3, 8, p1, 200, None, p2, 4100, C.byref(n2)) == -1
    assert _defaults(16, 3, 8, p1, 200, C.byref(n1), p2, 4100, None) == -1
    assert (b1 == 7.0).all() and (b2 == 7.0).all()   # (nothing written by a refused call)
    assert _defaults(16, 3, 8, p1, 129, C.byref(n1), p2, 257, C.byref(n2)) == 0 and (b1[129:] == 7.0).all() and (b2[257:] == 7.0).all()
    for bad in ((0, 3, 8), (16, 8, 3), (16, 4, 6)):
        with pytest.raises(m17hip.M17HipError):
            m17hip.wide_resample_default_taps(*bad)


# ---- 4: the ratio of a rate ------------------------------------------------------------------------------------------------------------------------------
RATIOS = {2048000: (16, 3, 8), 2400000: (10, 1, 5), 2500000: (5, 12, 125), 3000000: (5, 2, 25), 6000000: (5, 1, 25), 10000000: (5, 3, 125),
          250000: (1, 24, 125), 48000: (1, 1, 1)}


def test_the_ratio_of_a_rate():
    for rate, e in RATIOS.items():
        got = m17hip.wide_resample_ratio(rate)
        assert got == e, (rate, got)
        d1, up, down = got
        assert rate * up == 48000 * d1 * down and gcd(up, down) == 1
    # 1.024, 2.56, 8 and 20 MSPS of the header's table: whatever the split, the rate is the configuration's
    for rate in (1024000, 2560000, 8000000, 20000000, 96000, 768000):
        d1, up, down = m17hip.wide_resample_ratio(rate)
        assert rate * up == 48000 * d1 * down and 1 <= d1 <= 16 and 1 <= up <= min(down, 32) and down <= 125 and gcd(up, down) == 1, rate


def test_the_ratio_refuses_what_no_configuration_has():
    lib = m17hip.load_library()
    d1, up, down = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
    for rate in (0, 2000001, 47999, 24000, 1000, 48000 * 16 * 127, 44100):   # up above 32, below 48 kSPS, a prime factor no stage takes
        assert lib.m17hip_wide_resample_ratio(C.c_uint32(rate), C.byref(d1), C.byref(up), C.byref(down)) == -1, rate
    assert (d1.value, up.value, down.value) == (9, 9, 9)
    assert lib.m17hip_wide_resample_ratio(C.c_uint32(2048000), None, C.byref(up), C.byref(down)) == -1
    assert lib.m17hip_wide_resample_ratio(C.c_uint32(2048000), C.byref(d1), None, C.byref(down)) == -1
    assert lib.m17hip_wide_resample_ratio(C.c_uint32(2048000), C.byref(d1), C.byref(up), None) == -1
    for bad in (2000001, 0, -5, 1 << 32):
        with pytest.raises(m17hip.M17HipError):
            m17hip.wide_resample_ratio(bad)


# ---- 5: blocks -------------------------------------------------------------------------------------------------------------------------------------------
BLOCK_GROUPS = (1, 2, 85, 1, 100, 3, 67)


@pytest.mark.parametrize("case", [(8, 3, 16, 65, 513), (3, 5, 7, 7, 11)], ids=lambda c: "{}_{}over{}_{}_{}".format(*c))
@pytest.mark.parametrize("start", [0, (1 << 32) - 700], ids=["zero", "across_2^32"])
def test_a_feed_cut_at_block_boundaries_gives_the_words_of_the_uncut_feed(case, start):
    R1, U, D, L1, L2 = case
    rng = np.random.default_rng(6152 + D)
    cuts = np.cumsum((0,) + BLOCK_GROUPS).tolist()
    x = rng.integers(-20000, 20001, size=(cuts[-1] * R1 * D, 2)).astype(np.int16)
    taps1, taps2 = _taps(rng, L1), _taps(rng, L2)
    fcw = m17hip.wide_fcw(31000.0, R1 * D / U)
    whole = rl.Resampler(taps1, R1, U, D, taps2, fcw, 1.25, count=start).block(x)
    assert whole.size == cuts[-1] * U
    t = rl.Resampler(taps1, R1, U, D, taps2, fcw, 1.25, count=start)
    parts = [t.block(x[a * R1 * D: b * R1 * D]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [p.size for p in parts] == [U * g for g in BLOCK_GROUPS]
    assert np.array_equal(_u32(np.concatenate(parts)), _u32(whole))
    other = rl.Resampler(taps1, R1, U, D, taps2, fcw, 1.25, count=start + 1).block(x)
    assert not np.array_equal(_u32(other), _u32(whole))   # (the count matters)


# ---- 6: end to end at 2.048 MSPS on the host form alone --------------------------------------------------------------------------------------------------
KINDS = (1, 2, 4)   # stream, packet, packet with FCS
CH_R1, CH_U, CH_D = 8, 3, 16
OFFSETS = (-762500.0, 12500.0, 25000.0)
# tests/test_wide2_input.py's noise density (sigma 300 at 5 x 48 kSPS) at 128 / 3 x 48 kSPS
SIGMA = 300.0 * np.sqrt(128.0 / 3.0 / 5.0)
CLIPPED_CAP = 0.001


def source_2048k(basebands, seed=1):
    """Three transmissions in one 2.048 MSPS int16 source: made at 128 x 48 kSPS, every third sample kept (a constant-envelope signal may be thinned), noise
    added at the thinned rate, rounded; cut to whole groups of down * decim1 samples."""
    x = wl.wideband(basebands, OFFSETS, 128, fmt=wl.IQ_F32, sigma=0.0)[::3].astype(np.complex128)
    x = x[: x.size // (CH_R1 * CH_D) * (CH_R1 * CH_D)]
    rng = np.random.default_rng(seed)
    x = x + SIGMA * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return np.clip(np.rint(np.stack([x.real, x.imag], axis=-1)), -32768, 32767).astype(np.int16)


def _good(recs):
    r = recs[(recs["cost"] < 30) & (recs["frame_type"] != LICH)]
    return [(int(t), bytes(p)) for t, p in zip(r["frame_type"], r["payload"])]


def test_three_transmissions_in_one_2048k_source_carry_their_basebands_frames():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in KINDS]
    assert 48000 * CH_R1 * CH_D == 2048000 * CH_U
    x = source_2048k(bb)
    clipped = float(((x == -32768) | (x == 32767)).any(axis=-1).mean())
    assert clipped <= CLIPPED_CAP, clipped
    taps1, taps2 = m17hip.wide_resample_default_taps(CH_R1, CH_U, CH_D)
    for s, f in zip(bb, OFFSETS):
        expect = _good(ol.demod(s)[0])
        y = rl.resample(x, taps1, CH_R1, CH_U, CH_D, taps2, m17hip.wide_fcw(f, CH_R1 * CH_D / CH_U))
        recs = fl.demod(y)[0]
        got = _good(recs)
        print(f"{f} Hz: {len(got)} records, highest cost {max(int(c) for c in recs['cost'][(recs['cost'] < 30) & (recs['frame_type'] != LICH)])}")
        assert len(got) == 7 and [p for _, p in got] == [p for _, p in expect], (f, len(got), len(expect))


# ---- 7: exports, refusals and the Python layer -----------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_resample", "m17hip_wide_resample_default_taps", "m17hip_wide_resample_ratio"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 615
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_resample) and callable(m17hip.wide_resample_default_taps) and callable(m17hip.wide_resample_ratio)
    assert m17hip.KERNELS["resample"] == 13 and m17hip.KERNELS["survey"] == 12
    assert m17hip.wide_fcw(512000.0, 16 * 8 / 3) == 1 << 30 and m17hip.wide_fcw(-1024000.0, 128 / 3) == -(1 << 31)


def test_null_context_is_refused_by_wide_resample():
    lib = m17hip.load_library()
    taps = np.ones(1, dtype=np.float32)
    assert lib.m17hip_wide_resample(C.c_void_p(), C.c_uint32(1), C.c_uint32(16), ol._p(taps), C.c_uint32(1), C.c_uint32(3), C.c_uint32(8), ol._p(taps),
                                    C.c_uint32(1), C.c_int(1)) == -1
    assert lib.m17hip_wide_resample(C.c_void_p(), C.c_uint32(1), C.c_uint32(16), None, C.c_uint32(0), C.c_uint32(3), C.c_uint32(8), None, C.c_uint32(0),
                                    C.c_int(1)) == -1


def test_python_refuses_a_block_that_is_no_whole_number_of_groups():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the array is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    ctx._wide, ctx._wide_up = (2, 128, m17hip.IQ_I16), 3   # what wide_resample(2, 16, 3, 8) leaves: rows are multiples of 128 samples, 3 outputs each
    for bad in (np.zeros((2, 127, 2), dtype=np.int16), np.zeros((2, 192, 2), dtype=np.int16), np.zeros((1, 128, 2), dtype=np.int16),
                np.zeros((2, 128, 2), dtype=np.uint8), np.zeros((2, 128), dtype=np.complex64)):
        with pytest.raises(TypeError):
            ctx.upload_wide(bad)


# (decim1, up, down, ntaps1, ntaps2) -> (G, Q, LDS bytes) of every shape the device tests of the tile's forms, of the count across 2^32 and of the calls under
# the resampler rest on (tests/test_gpu_resample_tiles.py, test_gpu_wide_count_wrap.py, test_gpu_call_orders_resample.py): those choose their block sizes from
# G, so a rule that gives another tile fails here and there, and does not go on passing without its edges.  The last but one takes every byte of the LDS.
TILES = {(2, 2, 3, 5, 7): (255, 64, 14392), (3, 5, 6, 7, 11): (255, 64, 28696), (2, 2, 3, 5, 12): (255, 64, 14392), (2, 3, 4, 9, 24): (255, 64, 18520),
         (1, 3, 4, 1, 25): (255, 64, 16440), (1, 3, 4, 1, 23): (255, 64, 16408),
         (1, 32, 33, 1, 265): (121, 64, 65248), (1, 12, 31, 1, 249): (183, 64, 65264), (1, 12, 23, 1, 185): (226, 64, 65528), (1, 32, 91, 1, 729): (63, 64, 64784),
         (16, 2, 115, 256, 4096): (19, 57, 65464), (16, 2, 15, 129, 4096): (116, 63, 65512), (16, 2, 7, 256, 4096): (243, 58, 65536),
         (16, 3, 8, 33, 65): (255, 64, 55672), (16, 3, 8, 129, 257): (255, 64, 56952), (5, 12, 125, 41, 4001): (47, 64, 65088)}


def test_the_restated_tile_rule():
    """resample_lib.tile against the figures the kernel's comment and NOTES.md record, and over every accepted shape at the longest filters: there is a tile,
    it fits 64 KB, and a tile of one group with one u per chain would fit too.  TILES: the shapes the device tests choose their edges from."""
    for (R1, U, D, L1, L2), e in TILES.items():
        assert rl.tile(L1, R1, L2, U, D) == e, (R1, U, D, L1, L2)
    assert max(e[2] for e in TILES.values()) == rl.LDS_LIMIT
    table = {(16, 3, 8, 129, 257): (255, 64), (10, 1, 5, 81, 161): (255, 64), (5, 12, 125, 41, 4001): (47, 64), (16, 1, 125, 256, 4096): (13, 34),
             (16, 32, 125, 256, 4096): (22, 64)}
    for (R1, U, D, L1, L2), e in table.items():
        G, Q, lds = rl.tile(L1, R1, L2, U, D)
        assert (G, Q) == e and lds <= 65536, (R1, U, D, G, Q, lds)
    for D in range(1, 126):
        for U in (u for u in range(1, min(D, 32) + 1) if gcd(u, D) == 1):
            G, Q, lds = rl.tile(256, 16, 4096, U, D)
            assert 1 <= G <= 255 and 1 <= Q <= 64 and lds <= 65536, (U, D, G, Q, lds)


HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not present")
def test_the_restated_tile_rule_is_the_librarys(tmp_path):
    """resample_lib.tile is a RESTATEMENT, and the device tests choose their blocks' sizes from it: tests/cxx/resample_tile.cpp includes
    csrc/m17_resample_kernels.hpp and prints what resample_groups, resample_q and resample_lds_bytes themselves give (host code, no HIP call).  Held against
    the restatement over TILES, every accepted ratio at the longest filters, and 300 random accepted shapes."""
    exe = tmp_path / "resample_tile"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(iq.ROOT, "m17-cxx-demod_amd", "csrc"),
                        "-I", os.path.join(iq.ROOT, "m17-cxx-demod_amd", "include"), "-I", os.path.join(iq.ROOT, "include"),
                        os.path.join(iq.ROOT, "tests", "cxx", "resample_tile.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    shapes = list(TILES)
    shapes += [(16, U, D, 256, 4096) for D in range(1, 126) for U in range(1, min(D, 32) + 1) if gcd(U, D) == 1]
    rng = np.random.default_rng(6171)
    swept = len(shapes)
    while len(shapes) < swept + 300:
        R1, U, D, L1, L2 = (int(rng.integers(lo, hi + 1)) for lo, hi in ((1, 16), (1, 32), (1, 125), (1, 256), (1, 4096)))
        if U <= D and gcd(U, D) == 1:
            shapes.append((R1, U, D, L1, L2))
    out = subprocess.run([str(exe)] + [str(v) for s in shapes for v in s], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert len(got) == len(shapes)
    for (R1, U, D, L1, L2), g in zip(shapes, got):
        assert rl.tile(L1, R1, L2, U, D) == g, (R1, U, D, L1, L2, g)


def test_example_takes_a_2048k_source_by_its_rate():
    """examples/m17-demod-gpu --wide-i16 / --wide-u8 --rate 2048000 --offset-hz F prints what --float32 prints on the host form's floats at 16 x 3 / 8
    (M17_DEMOD_DEVICE=cpu: the scalar demodulator over core::ddc_resample, a group of 3 outputs at a time; on the GPU path the same class goes through
    m17hip_wide_resample, tests/test_gpu_resample_input.py).  --rate excludes --decim, --decim2 and --raster."""
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ, M17_DEMOD_DEVICE="cpu")
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in KINDS]
    assert m17hip.wide_resample_ratio(2048000) == (16, 3, 8)
    taps1, taps2 = m17hip.wide_resample_default_taps(16, 3, 8)
    x16 = source_2048k(bb)
    x8 = np.clip(np.rint(x16.astype(np.float64) / 160.0 + 127.5), 0, 255).astype(np.uint8)
    for x, flag, gain, f in ((x16, "--wide-i16", "1", OFFSETS[1]), (x8, "--wide-u8", "2", OFFSETS[0])):
        y = rl.resample(x, taps1, 16, 3, 8, taps2, m17hip.wide_fcw(f, 128 / 3), float(gain))
        got = subprocess.run([exe, flag, "--rate", "2048000", "--offset-hz", str(int(f)), "--iq-gain", gain], input=x.tobytes(), capture_output=True,
                             env=env, check=True).stdout
        exp = subprocess.run([exe, "--float32"], input=y.tobytes(), capture_output=True, env=env, check=True).stdout
        assert got == exp and len(got.splitlines()) >= 6, flag
    for bad in (["--rate", "2048000", "--decim", "16"], ["--rate", "2048000", "--decim2", "4"], ["--rate", "2048000", "--raster", "64"],
                ["--rate", "2000001"], ["--rate", "0"], ["--rate", "2048000", "--offset-hz", "1100000"]):
        assert subprocess.run([exe, "--wide-i16"] + bad, input=b"", capture_output=True, env=env).returncode == 2, bad
    assert subprocess.run([exe, "--rate", "2048000"], input=b"", capture_output=True, env=env).returncode == 2
