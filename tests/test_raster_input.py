"""CPU-only: wideband IQ input on a channel raster (ABI 611, include/m17hip.h: m17hip_wide_raster — the polyphase channeliser).  1: the HOST form
(detail/core.h's chan_fold / chan_pass1 / chan_pass2 under the host compiler, tests/cxx/raster_oracle.cpp) against a plain float64 statement of the DIRECT
sum, within a derived bound that a wrong decimation phase, a residue shifted by one and a fold begun at the wrong tap each miss.  2: the small shapes where
indexing can go wrong.  3: a feed cut anywhere gives the words of the uncut feed, and only the count mod M enters.  4: with the oscillator on the raster the
single-stage tuner computes the same z, within the sum of the two bounds.  5: the twiddle table and the default taps are what the header says.  6: the
feature means something — three FM transmissions in one 2.4 MSPS source carry their basebands' frames.  7: what the new calls promise without a GPU, and the
example on the host form of the demodulator class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import raster_lib as rl
import wide2_lib as w2
import wide_lib as wl

LICH = 1
GAIN = 1.25


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bin_word(b, M):
    """The frequency word of bin b of M: exact where M divides 2^32, else the nearest word (a carrier is put there, nothing is tuned with it)."""
    return int(round(b * 4294967296.0 / M))


# ---- 1: against float64 ---------------------------------------------------------------------------------------------------------------------------------
# raster_lib.chan_f64 on wide_lib.carriers: 600 outputs, a carrier 1 kHz off the centre of EVERY tested bin (so that |z| stands above the floor the phase
# rule needs), noise of sigma 100; wide_lib.hamming_taps.  The bounds are DERIVED (raster_lib.f64_bound's docstring):
#   |z_host - z_f64| <= sqrt 2 2^-24 scale (ceil(L / M) + 2 M1 + 2 M2 + 2), scale = sum|taps| max|x|;
#   |y_host - y_f64| (mod 2 pi) <= gain (2 bound / min|z| + 2^-20) wherever z[n] and z[n-1] of the reference both exceed 8 bound (wide_lib.f64_check_y's rule).
# Once the filter has filled at most 1 % of a case's outputs may fall under that floor, and at most 0.001 of the input samples may lie on a rail: both
# asserted on the reference and the input alone, before the host form is looked at.
# (M, decim, taps, bins)
F64_CASES = [(6, 4, 13, (-3, 0, 2)), (12, 4, 5, (-6, 1, 5)), (13, 3, 40, (-6, 0, 6)), (64, 5, 161, (-32, -1, 0, 31)), (192, 50, 1601, (-96, -61, 1, 2, 95)),
             (256, 64, 4096, (-128, 3, 127)), (240, 60, 1921, (-120, 7, 119)), (120, 25, 801, (-60, 59))]
F64_N = 600
F64_EXCLUDED_CAP = 0.01
RAIL_CAP = 0.001


def _f64_input(M, R, bins, fmt, seed):
    x = wl.carriers(R, [_bin_word(b, M) for b in bins], F64_N, fmt, seed=seed, offset_hz=1000.0)
    if fmt != wl.IQ_F32:
        rails = (-32768, 32767) if fmt == wl.IQ_I16 else (0, 255)
        assert float(((x == rails[0]) | (x == rails[1])).any(axis=-1).mean()) <= RAIL_CAP
    return x


@pytest.mark.parametrize("fmt", [wl.IQ_I16, wl.IQ_F32], ids=["i16", "f32"])
@pytest.mark.parametrize("case", F64_CASES, ids=["M{}_R{}_L{}".format(*c[:3]) for c in F64_CASES])
def test_the_channeliser_is_within_derived_bounds_of_float64(case, fmt):
    M, R, L, bins = case
    taps = wl.hamming_taps(L)
    x = _f64_input(M, R, bins, fmt, 6111 + M)
    fill = -(-L // R)   # outputs until the filter has filled
    y, z = rl.Raster(taps, R, M, bins, GAIN).block(x, want_z=True)
    worst = [0.0, 0.0, 0.0]
    for i, b in enumerate(bins):
        y64, z64, scale = rl.chan_f64(x, taps, R, M, b, GAIN)
        bound = rl.f64_bound(scale, L, M)
        excluded = 1.0 - float(w2.f64_ok(z64, bound)[fill:].mean())
        assert excluded <= F64_EXCLUDED_CAP, (case, b, excluded)
        ez, ey, _ = w2.f64_errors(y[i], z[i], y64, z64, bound, GAIN)
        assert y[i][0] == 0.0 and y64[0] == 0.0
        assert ez <= 1.0 and ey <= 1.0, (case, b, ez, ey)
        worst = [max(p, q) for p, q in zip(worst, (ez, ey, excluded))]
    print(f"channeliser vs float64, M {M} decim {R} taps {L}: z error {worst[0]:.4f} of its bound, y error {worst[1]:.4f}, excluded {100 * worst[2]:.2f} %")


def test_a_wrong_phase_a_shifted_residue_and_a_wrong_first_tap_each_miss_the_z_bound():
    """The float64 statement with sample n R + R - 2 newest in place of the last of each group, with the phase taken from the sample index + 1, and with
    tap i + 1 where tap i belongs: the host form is far outside the bound it meets against the right statement."""
    M, R, L, b = 192, 50, 1601, -61
    taps = wl.hamming_taps(L)
    x = _f64_input(M, R, (b,), wl.IQ_I16, 6112)
    _, z = rl.Raster(taps, R, M, [b], GAIN).block(x, want_z=True)
    _, right, scale = rl.chan_f64(x, taps, R, M, b, GAIN)
    wrong = [rl.chan_f64(x, taps, R, M, b, GAIN, **kw)[1] for kw in ({"keep": R - 2}, {"residue": 1}, {"tap0": 1})]
    bound = rl.f64_bound(scale, L, M)
    e = [float(np.abs(z[0] - r).max()) / bound for r in [right] + wrong]
    print(f"z error over its bound: right {e[0]:.4f}, one sample early {e[1]:.1f}, residue + 1 {e[2]:.1f}, fold from tap 1 {e[3]:.1f}")
    assert e[0] <= 1.0
    assert min(e[1:]) > 1.0


def test_the_fold_chains_run_from_tap_i0_upwards():
    """M = 2, decim 6, six taps of 1: residue r of the one output (newest sample m = 5) folds the three samples of parity r, newest first.  With the values
    2^24, 1, -2^24 in that order the chain gives 0, from the other end 1 (a tie to even loses the 1); the imaginary parts hold them the other way round,
    so one output shows both.  Bin 0 is w[0] + w[1], bin -1 is w[0] - w[1]; w[0] = 0 here."""
    big = float(1 << 24)
    f32 = np.float32
    up = (f32(big) + f32(1.0)) + f32(-big)
    down = (f32(-big) + f32(1.0)) + f32(big)
    assert up == 0.0 and down == 1.0
    # oldest first: samples 0..5; parity 1 (newest m = 5, then 3, then 1) holds big, 1, -big in the real part and the reverse in the imaginary one
    x = np.zeros(6, dtype=np.complex64)
    x[5], x[3], x[1] = big - 1j * big, 1.0 + 1.0j, -big + 1j * big
    _, z = rl.Raster(np.ones(6, dtype=np.float32), 6, 2, [0, -1], 1.0).block(x, want_z=True)
    assert z.shape == (2, 1)
    assert z[0, 0].real == up and z[0, 0].imag == down        # bin 0: w[1] + w[0], w[0] = 0
    assert z[1, 0].real == -up and z[1, 0].imag == -down      # bin -1: w[0] - w[1]


# ---- 2: small shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rl.SMALL, ids=["M{}_R{}_L{}".format(*s) for s in rl.SMALL])
def test_small_shapes_every_bin_against_float64(shape):
    """6 = 3 x 2 at decim 4 with 7 and 13 taps; M = 12 with 5 taps (seven residues get no tap); decim = M; decim > M; gcd(decim, M) = 1 — every bin, random
    taps and samples, 200 outputs from a count that is no multiple of M: |z - z_f64| within the derived bound (no carrier here: z alone is judged)."""
    M, R, L = shape
    rng = np.random.default_rng(6113 + M + R + L)
    taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    x = rng.integers(-20000, 20001, size=(200 * R, 2)).astype(np.int16)
    bins = list(range(-(M // 2), (M - 1) // 2 + 1))
    assert rl.factor(M) == rl.factor_stated(M) and rl.factor(M) is not None
    if L < M:
        assert sum(1 for r in range(M) if not any(i % M == r for i in range(L))) == M - L
    for count in (0, 5):
        _, z = rl.Raster(taps, R, M, bins, 1.0, count=count).block(x, want_z=True)
        for i, b in enumerate(bins):
            _, z64, scale = rl.chan_f64(x, taps, R, M, b, 1.0, count=count)
            assert float(np.abs(z[i] - z64).max()) <= rl.f64_bound(scale, L, M), (shape, b, count)


# ---- 3: block cuts and the count ------------------------------------------------------------------------------------------------------------------------
CUT_T, CUT_M, CUT_R, CUT_L = 1500, 192, 50, 257
CUT_CUTS = np.cumsum([0, 1, 2, 255, 1024]).tolist() + [CUT_T]
CUT_BINS = (-96, -61, 0, 1, 95)


@pytest.fixture(scope="module")
def cut_case():
    rng = np.random.default_rng(6114)
    x = rng.integers(-20000, 20001, size=(CUT_T * CUT_R, 2)).astype(np.int16)
    taps = (rng.standard_normal(CUT_L) / np.sqrt(CUT_L)).astype(np.float32)
    x.setflags(write=False)
    return x, taps


@pytest.mark.parametrize("start", [0, 7, (1 << 32) - 700], ids=["zero", "seven", "across_2^32"])
def test_a_feed_cut_at_block_boundaries_gives_the_words_of_the_uncut_feed(cut_case, start):
    x, taps = cut_case
    R = CUT_R
    assert len({(start + a * R) % CUT_M for a in CUT_CUTS[:-1]}) == len(CUT_CUTS) - 1   # (decim is no multiple of M: every boundary has another count mod M)
    whole = rl.Raster(taps, R, CUT_M, CUT_BINS, GAIN, count=start).block(x)
    t = rl.Raster(taps, R, CUT_M, CUT_BINS, GAIN, count=start)
    parts = [t.block(x[a * R: b * R]) for a, b in zip(CUT_CUTS[:-1], CUT_CUTS[1:])]
    assert np.array_equal(_u32(np.concatenate(parts, axis=1)), _u32(whole))
    # ... and the count matters: the same blocks from another count are other words (in bin 0 too: its phase is always 1, but the taps fall into other
    # residues, so the same sum is rounded in another order)
    other = rl.Raster(taps, R, CUT_M, CUT_BINS, GAIN, count=start + 1).block(x)
    for i, b in enumerate(CUT_BINS):
        assert not np.array_equal(_u32(other[i]), _u32(whole[i])), b


def test_only_the_count_mod_M_enters():
    rng = np.random.default_rng(6115)
    x = rng.integers(-20000, 20001, size=(300 * CUT_R, 2)).astype(np.int16)
    taps = (rng.standard_normal(CUT_L) / np.sqrt(CUT_L)).astype(np.float32)
    c = (1 << 32) + 5
    assert c % CUT_M == 69 and (c & 0xFFFFFFFF) % CUT_M == 5   # (2^32 mod 192 = 64: a count truncated to 32 bits is 64 bins off)
    a = rl.Raster(taps, CUT_R, CUT_M, CUT_BINS, GAIN, count=c).block(x)
    b = rl.Raster(taps, CUT_R, CUT_M, CUT_BINS, GAIN, count=c % CUT_M).block(x)
    t = rl.Raster(taps, CUT_R, CUT_M, CUT_BINS, GAIN, count=c & 0xFFFFFFFF).block(x)
    assert np.array_equal(_u32(a), _u32(b)) and not np.array_equal(_u32(a), _u32(t))


# ---- 4: against the single-stage tuner ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 16])
def test_the_single_stage_tuner_on_the_raster_computes_the_same_z(R):
    """M = 64: bin k is the frequency word k 2^26 exactly, so the tuner's z and the channeliser's are two float32 evaluations of one sum: they differ by at
    most the sum of their two derived bounds."""
    M, L = 64, 32 * R + 1
    taps = wl.hamming_taps(L)
    bins = (-32, -17, -1, 0, 1, 31)
    x = _f64_input(M, R, bins, wl.IQ_I16, 6116 + R)
    _, z = rl.Raster(taps, R, M, bins, GAIN).block(x, want_z=True)
    scale = float(np.abs(taps.astype(np.float64)).sum() * np.abs(rl.samples_f64(x)).max())
    both = rl.f64_bound(scale, L, M) + wl.f64_bound(scale, L)
    for i, k in enumerate(bins):
        _, zt = wl.Tuner(taps, R, k << 26, GAIN).block(x, want_z=True)
        e = float(np.abs(z[i].astype(np.complex128) - zt.astype(np.complex128)).max())
        assert e <= both, (R, k, e / both)
        assert np.abs(zt).max() > 100 * both   # (there is a signal to agree on)


# ---- 5: twiddles and default taps -----------------------------------------------------------------------------------------------------------------------
ACCEPTED = (48, 64, 96, 120, 128, 144, 192, 240, 256)


@pytest.mark.parametrize("M", ACCEPTED + (1, 2, 6, 9, 12, 13, 16))
def test_twiddles_are_exact_on_the_axes_conjugate_symmetric_and_within_half_an_ulp(M):
    tw = m17hip.wide_raster_twiddles(M)
    assert tw.dtype == np.complex64 and tw.shape == (M,)
    ref = rl.twiddles_f64(M)
    assert float(np.abs(tw.real.astype(np.float64) - ref.real).max()) <= 2.0 ** -25
    assert float(np.abs(tw.imag.astype(np.float64) - ref.imag).max()) <= 2.0 ** -25
    for j in range(M):
        if (4 * j) % M == 0:
            assert (tw[j].real, tw[j].imag) == {0: (1.0, 0.0), 1: (0.0, -1.0), 2: (-1.0, 0.0), 3: (0.0, 1.0)}[4 * j // M], j
        if j:
            assert _u32(tw[M - j].real) == _u32(tw[j].real), j
            assert tw[M - j].imag == -tw[j].imag, j


def test_the_factors():
    for M in range(0, 300):
        assert rl.factor(M) == rl.factor_stated(M), M
    for M in ACCEPTED:
        m1, m2 = rl.factor(M)
        assert m1 * m2 == M and m2 <= m1 <= 16
    assert rl.factor(192) == (16, 12) and rl.factor(6) == (3, 2) and rl.factor(13) == (13, 1)
    for M in (0, 17, 34, 250, 257, 512):
        assert rl.factor(M) is None, M


def test_default_taps_are_the_tuners_up_to_16_and_the_same_formula_beyond():
    for R in range(1, 17):
        assert np.array_equal(_u32(m17hip.wide_raster_default_taps(R)), _u32(m17hip.wide_default_taps(R)))
    for R in (17, 50, 64):
        taps = m17hip.wide_raster_default_taps(R)
        L = 32 * R + 1
        assert taps.dtype == np.float32 and taps.size == L
        t = np.arange(L, dtype=np.float64) - 0.5 * (L - 1)
        fc = 5500.0 / (48000.0 * R)
        h = 2.0 * fc * np.sinc(2.0 * fc * t) * (0.42 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / (L - 1)) + 0.08 * np.cos(4.0 * np.pi * np.arange(L) / (L - 1)))
        assert float(np.abs(taps.astype(np.float64) - h / h.sum()).max()) <= 2.0 ** -24 * float(np.abs(h / h.sum()).max()) + 1e-12
    n = C.c_uint32(0)
    buf = np.full(2100, 7.0, dtype=np.float32)
    lib = m17hip.load_library()
    for R in (0, 65):
        assert lib.m17hip_wide_raster_default_taps(C.c_uint32(R), ol._p(buf), C.c_uint32(buf.size), C.byref(n)) == -1
    assert lib.m17hip_wide_raster_default_taps(C.c_uint32(50), ol._p(buf), C.c_uint32(1600), C.byref(n)) == -1 and n.value == 1601
    assert lib.m17hip_wide_raster_default_taps(C.c_uint32(50), None, C.c_uint32(0), C.byref(n)) == -1 and n.value == 1601
    assert lib.m17hip_wide_raster_default_taps(C.c_uint32(50), ol._p(buf), C.c_uint32(buf.size), None) == -1
    assert (buf == 7.0).all()
    assert lib.m17hip_wide_raster_default_taps(C.c_uint32(64), ol._p(buf), C.c_uint32(2049), C.byref(n)) == 0 and n.value == 2049 and (buf[2049:] == 7.0).all()
    with pytest.raises(m17hip.M17HipError):
        m17hip.wide_raster_default_taps(65)


# ---- 6: end to end at 2.4 MSPS on the host form alone ---------------------------------------------------------------------------------------------------
KINDS = (1, 2, 4)   # stream, packet, packet with FCS
E2E_R, E2E_M = 50, 192
OFFSETS = (-762500.0, 12500.0, 25000.0)   # tests/test_wide2_input.py's: bins -61, 1 and 2 of the 12.5 kHz raster
SIGMA = 300.0 * np.sqrt(10.0)
CLIPPED_CAP = 0.001


def _good(recs):
    r = recs[(recs["cost"] < 30) & (recs["frame_type"] != LICH)]
    return [(int(t), bytes(p)) for t, p in zip(r["frame_type"], r["payload"])]


@pytest.fixture(scope="module")
def basebands():
    out = []
    for kind in KINDS:
        s = ol.generate(ol.gen_params(seed=1, kind=kind, lead_in=9600, n_frames=6, tail=4800))
        s.setflags(write=False)
        out.append((s, _good(ol.demod(s)[0])))
    return out


@pytest.mark.parametrize("case", [(wl.IQ_I16, 6000.0, 0.0), (wl.IQ_I16, 6000.0, SIGMA), (wl.IQ_U8, 40.0, 0.0)], ids=["i16_clean", "i16_noise", "u8_clean"])
def test_three_transmissions_in_one_2400k_source_carry_their_basebands_frames(basebands, case):
    fmt, amplitude, sigma = case
    bins = [m17hip.wide_bin(f, E2E_R, E2E_M) for f in OFFSETS]
    assert bins == [-61, 1, 2]
    x = wl.wideband([s for s, _ in basebands], OFFSETS, E2E_R, amplitude=amplitude, sigma=sigma, seed=1, fmt=fmt)
    rails = (-32768, 32767) if fmt == wl.IQ_I16 else (0, 255)
    clipped = float(((x == rails[0]) | (x == rails[1])).any(axis=-1).mean())
    assert clipped <= CLIPPED_CAP, clipped
    y = rl.chan(x, m17hip.wide_raster_default_taps(E2E_R), E2E_R, E2E_M, bins)
    for (s, expect), row in zip(basebands, y):
        got = _good(fl.demod(row)[0])
        assert len(expect) >= 7 and got == expect, (case, len(got), len(expect))


# ---- 7: exports, refusals, the Python layer and the example ---------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_raster_default_taps", "m17hip_wide_raster_twiddles", "m17hip_wide_raster", "m17hip_wide_raster_channels"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 611
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for f in (m17hip.Context.wide_raster, m17hip.Context.wide_raster_channels, m17hip.wide_raster_default_taps, m17hip.wide_raster_twiddles, m17hip.wide_bin):
        assert callable(f)
    assert m17hip.KERNELS["channelise"] == 11 and m17hip.KERNELS["tune2"] == 10
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(iq.ROOT, "m17-cxx-demod_amd", "libm17hip.so")], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(iq.ROOT, "include", "m17hip.h")).read()
    for name in NEW:
        assert f" T {name}\n" in out and f"int {name}(" in header, name


def test_wide_bin():
    assert m17hip.wide_bin(12500.0, 50, 192) == 1 and m17hip.wide_bin(-762500.0, 50, 192) == -61 and m17hip.wide_bin(0.0, 50, 192) == 0
    assert m17hip.wide_bin(-1200000.0, 50, 192) == -96 and m17hip.wide_bin(1187500.0, 50, 192) == 95
    assert m17hip.wide_bin(-40000.0, 5, 6) == -1
    for hz in (6250.0, 12501.0, 1200000.0, -1212500.0):
        with pytest.raises(ValueError):
            m17hip.wide_bin(hz, 50, 192)


def test_refusals_that_need_no_context():
    lib = m17hip.load_library()
    taps = np.ones(1, dtype=np.float32)
    z32, i32 = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)
    assert lib.m17hip_wide_raster(C.c_void_p(), C.c_uint32(1), C.c_uint32(50), C.c_uint32(192), C.c_int(1), ol._p(taps), C.c_uint32(1)) == -1
    assert lib.m17hip_wide_raster(C.c_void_p(), C.c_uint32(1), C.c_uint32(50), C.c_uint32(192), C.c_int(1), None, C.c_uint32(0)) == -1
    assert lib.m17hip_wide_raster_channels(C.c_void_p(), ol._p(z32), ol._p(i32), C.c_uint32(1)) == -1
    buf = np.full(600, 7.0, dtype=np.float32)
    for M in (0, 17, 34, 257, 1024):   # (34 = 17 x 2: no two factors up to 16)
        assert lib.m17hip_wide_raster_twiddles(C.c_uint32(M), ol._p(buf), C.c_uint32(buf.size)) == -1, M
        with pytest.raises(m17hip.M17HipError):
            m17hip.wide_raster_twiddles(M)
    assert lib.m17hip_wide_raster_twiddles(C.c_uint32(192), ol._p(buf), C.c_uint32(383)) == -1
    assert lib.m17hip_wide_raster_twiddles(C.c_uint32(192), None, C.c_uint32(384)) == -1
    assert (buf == 7.0).all()
    assert lib.m17hip_wide_raster_twiddles(C.c_uint32(192), ol._p(buf), C.c_uint32(384)) == 0 and (buf[384:] == 7.0).all() and buf[0] == 1.0


def test_python_refuses_a_block_that_does_not_fit_the_raster_configuration():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the array is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    ctx._wide = (2, 50, m17hip.IQ_U8)   # what wide_raster(2, 50, 192, IQ_U8) leaves: rows are multiples of 50 samples
    for bad in (np.zeros((2, 40, 2), dtype=np.uint8), np.zeros((2, 99, 2), dtype=np.uint8), np.zeros((1, 100, 2), dtype=np.uint8),
                np.zeros((2, 100, 2), dtype=np.int16), np.zeros((2, 100), dtype=np.complex64)):
        with pytest.raises(TypeError):
            ctx.upload_wide(bad)
    with pytest.raises(ValueError):
        ctx.wide_raster_channels([0, 1], [0])


def test_example_takes_a_bin_of_a_2400k_raster(basebands):
    """examples/m17-demod-gpu --wide-u8 / --wide-i16 --decim 50 --raster 192 --bin B on a 2.4 MSPS source prints what --float32 prints on the host form's
    floats (M17_DEMOD_DEVICE=cpu: the scalar demodulator class, whose wide_raster computes the same words; on the GPU path the same class goes through
    m17hip_wide_raster)."""
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ, M17_DEMOD_DEVICE="cpu")
    taps = m17hip.wide_raster_default_taps(E2E_R)
    for fmt, flag, amplitude, gain, b in ((wl.IQ_U8, "--wide-u8", 40.0, "2", 1), (wl.IQ_I16, "--wide-i16", 6000.0, "1", -61)):
        x = wl.wideband([s for s, _ in basebands], OFFSETS, E2E_R, amplitude=amplitude, sigma=0.0, fmt=fmt)
        n = 24000   # (a short file: the first outputs of the feed, through the first frames)
        x = x[: n * E2E_R]
        y = rl.chan(x, taps, E2E_R, E2E_M, [b], float(gain))[0]
        got = subprocess.run([exe, flag, "--decim", "50", "--raster", "192", "--bin", str(b), "--iq-gain", gain], input=x.tobytes(), capture_output=True,
                             env=env, check=True).stdout
        exp = subprocess.run([exe, "--float32"], input=y.tobytes(), capture_output=True, env=env, check=True).stdout
        assert got == exp and len(got.splitlines()) >= 2, flag
    for bad in (["--raster", "34", "--bin", "0"], ["--raster", "192", "--bin", "96"], ["--raster", "192", "--bin", "-97"], ["--raster", "0", "--bin", "0"],
                ["--raster", "192", "--bin", "0", "--decim2", "5"]):
        assert subprocess.run([exe, "--wide-u8", "--decim", "50"] + bad, input=b"", capture_output=True, env=env).returncode == 2, bad
    assert subprocess.run([exe, "--wide-u8", "--decim", "65", "--raster", "192", "--bin", "0"], input=b"", capture_output=True, env=env).returncode == 2


# ---- 8: the inputs of tests/test_gpu_call_orders_raster.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i16", "u8"])
def test_reference_data_of_the_call_order_module_meets_its_premises(fmt):
    """tests/test_gpu_call_orders_raster.py's reference data built without a device — its sources (the same seed and length), the distinct channel set, the
    alternative tables — and the conditions on them its cases lean on, at a block 1 of 385 outputs and a block of 384 behind it (a prefix of the module's
    block 1: rows that differ here differ there): exactly one pair of channels has identical words and every other pair differs, in both blocks; under
    every alternative table each moved channel differs from the base table's, in block 1 and in the block behind; the count at the boundary is nonzero
    mod 192 and a feed that lost it has other words on every channel whose bin notices; and — over the module's whole block 1, on the nine channels that
    listen to a transmission — every transmission bin yields records."""
    import test_gpu_call_orders_raster as cr
    import test_gpu_call_orders_formats as par
    import copy
    n1, nb = cr.TB + 1, cr.TB
    assert sorted(set(cr.BINS.tolist())) == sorted(set(cr.TX_BINS) | set(cr._OTHERS)) and {-96, 0, 95} <= set(cr.BINS.tolist())
    assert [int(np.sum(cr.SRC == s)) for s in range(cr.S)] == [32, 32] and cr.ALL == 64 * cr.REP and cr.NS <= 256
    x = cr.sources(cr.FMTS[fmt])
    assert x.shape[1] == cr.TOTAL * cr.R and cr.REP * x[0].nbytes * cr.S <= 512 * 10 ** 6
    base = cr.feeds(x)
    y1 = base.block(0, n1)
    cr.one_pair_alike(y1)
    assert base.per_source[0].count == n1 * cr.R and (n1 * cr.R) % cr.M != 0 and ((cr.T1 + 1) * cr.R) % cr.M == (n1 * cr.R) % cr.M
    behind = copy.deepcopy(base)
    y2 = base.block(n1, n1 + nb)
    cr.one_pair_alike(y2)
    lost = copy.deepcopy(behind)
    for t in lost.per_source:
        t.count = 0
    notices = [c for c in range(64) if (cr.BINS[c] * n1 * cr.R) % cr.M != 0]
    assert len(notices) >= 60 and (_u32(lost.block(n1, n1 + nb)) != _u32(y2)).any(axis=1)[notices].all()
    for k in (1, 2, 3):
        who, src, bins = cr.table(k)
        assert who.size == 16 and (src[who] != cr.SRC[who]).all() and sorted(np.bincount(src).tolist()) == [16, 48]
        assert len({(int(s), int(b)) for s, b in zip(src, bins)}) < 63 and not {(int(s), int(b)) for s, b in zip(src, bins)} <= {(int(s), int(b)) for s, b in zip(cr.SRC, cr.BINS)}
        cr.moved_differ(y1, cr.feeds(x, src, bins).block(0, n1), who)
        other = copy.deepcopy(behind)
        other.src, other.bins = list(src), list(bins)
        cr.moved_differ(y2, other.block(n1, n1 + nb), who)
    tx = cr.TX_CHANNELS
    y = cr.feeds(x, cr.SRC[tx], cr.BINS[tx]).block(0, cr.T1)
    assert np.array_equal(_u32(y[:, :n1]), _u32(y1[tx]))
    rows = par.Expect(y).run(0, cr.T1)
    assert all(r.size > 0 for r in rows), [r.size for r in rows]
