"""CPU-only: wideband IQ input (ABI 609, include/m17hip.h: m17hip_wide_config, m17hip_wide_channels, m17hip_upload_wide and friends).  1: the
oscillator of the tuner's HOST form (detail/core.h under the host compiler, tests/cxx/wide_oracle.cpp) — exactly on the axes at the quarter phases, within
2^-21 of float64 over all 2^26 distinct inputs.  2: the phase of a sample is fcw * m modulo 2^32, so a feed cut anywhere gives the words of the uncut feed.
3: pins with no polynomial in them — a quarter-rate mix is a rotation by -j, a zero offset with one tap is iq_lib's discriminator, and the fma chains run
in the order i = 0 .. L - 1.  4: the feature means something — three FM transmissions in one int16 (and uint8) wideband, tuned by the host form and
demodulated by the float oracle, each carry the frames the int16 oracle finds in their baseband.  5: what the new calls promise without a GPU.  6: the
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
import wide_lib as wl

# the oscillator's error against float64: 2.8e-7 measured over all 2^26 inputs; asserted is the next power of two above it, which must not exceed 2^-17
# (half an LSB of a full-scale int16 sample: the oscillator adds less than the input's own quantisation)
NCO_BOUND = 2.0 ** -21
LICH = 1


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1: the oscillator ----------------------------------------------------------------------------------------------------------------------------
def test_oscillator_is_exactly_on_the_axes_at_the_quarter_phases():
    c, s = wl.nco(np.array([0, 1 << 30, 1 << 31, 3 << 30], dtype=np.uint32))
    assert c.tolist() == [1.0, 0.0, -1.0, 0.0] and s.tolist() == [0.0, 1.0, 0.0, -1.0]   # (zeroes of either sign compare equal)


def test_oscillator_is_within_the_bound_of_float64_over_all_inputs():
    worst = 0.0
    step = 1 << 22
    for k0 in range(0, 1 << 26, step):
        k = np.arange(k0, k0 + step, dtype=np.uint64)
        c, s = wl.nco((k << np.uint64(6)).astype(np.uint32))
        a = k.astype(np.float64) * (2.0 * np.pi / (1 << 26))
        worst = max(worst, float(np.abs(c - np.cos(a)).max()), float(np.abs(s - np.sin(a)).max()))
    print(f"nco: max abs error {worst:.3e} = 2^{np.log2(worst):.2f}")
    assert NCO_BOUND <= 2.0 ** -17
    assert NCO_BOUND / 2 < worst <= NCO_BOUND, worst


def test_oscillator_looks_at_the_upper_26_bits_only():
    rng = np.random.default_rng(609)
    p = rng.integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)
    c, s = wl.nco(p)
    for low in (0, 63, 21):
        c2, s2 = wl.nco((p & np.uint32(0xFFFFFFC0)) | np.uint32(low))
        assert np.array_equal(_u32(c), _u32(c2)) and np.array_equal(_u32(s), _u32(s2))


# ---- 2: the phase ----------------------------------------------------------------------------------------------------------------------------------
PH_T, PH_R, PH_L = 3000, 3, 25
PH_CUTS = np.cumsum([0, 1, 2, 255, 1024]).tolist() + [PH_T]


@pytest.fixture(scope="module")
def ph_case():
    rng = np.random.default_rng(6091)
    x = rng.integers(-20000, 20001, size=(PH_T * PH_R, 2)).astype(np.int16)
    taps = rng.standard_normal(PH_L).astype(np.float32) / np.float32(PH_L)
    x.setflags(write=False)
    return x, taps


@pytest.mark.parametrize("start", [0, (1 << 32) + 12345, (1 << 32) - 700], ids=["zero", "above_2^32", "across_2^32"])
def test_the_phase_of_sample_m_is_fcw_times_m(ph_case, start):
    """One tap of 1 and no decimation: z[m] is x[m] conj(nco(fcw m mod 2^32)), whatever the count was when the block began."""
    x, _ = ph_case
    fcw = -0x12345679
    t = wl.Tuner([1.0], 1, fcw, count=start)
    _, z = t.block(x[:4096], want_z=True)
    m = (np.arange(4096, dtype=np.uint64) + np.uint64(start)) & np.uint64(0xFFFFFFFF)
    p = ((m * np.uint64(fcw & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c, s = wl.nco(p)
    re, im = iq.cross(x[:4096, 0].astype(np.float32), x[:4096, 1].astype(np.float32), c, s)
    assert np.array_equal(_u32(z.real), _u32(re)) and np.array_equal(_u32(z.imag), _u32(im))


@pytest.mark.parametrize("start", [0, (1 << 32) + 12345], ids=["zero", "above_2^32"])
def test_a_feed_cut_at_block_boundaries_gives_the_words_of_the_uncut_feed(ph_case, start):
    x, taps = ph_case
    fcw = m17hip.wide_fcw(31000.0, PH_R)
    whole = wl.Tuner(taps, PH_R, fcw, 1.25, count=start).block(x)
    t = wl.Tuner(taps, PH_R, fcw, 1.25, count=start)
    parts = [t.block(x[a * PH_R: b * PH_R]) for a, b in zip(PH_CUTS[:-1], PH_CUTS[1:])]
    assert np.array_equal(_u32(np.concatenate(parts)), _u32(whole))
    # ... and the count matters: the same blocks from another count are other words
    other = wl.Tuner(taps, PH_R, fcw, 1.25, count=start + 1).block(x)
    assert not np.array_equal(_u32(other), _u32(whole))


# ---- 3: pins with no polynomial in them ---------------------------------------------------------------------------------------------------------------
def test_a_quarter_rate_mix_is_a_rotation_by_minus_j():
    rng = np.random.default_rng(6092)
    x = rng.integers(1, 30000, size=(4000, 2)).astype(np.int16) * rng.choice(np.array([-1, 1], dtype=np.int16), size=(4000, 2))
    _, z = wl.Tuner([1.0], 1, 1 << 30).block(x, want_z=True)
    xc = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    exp = xc * np.array([1, -1j, -1, 1j])[np.arange(4000) % 4]
    assert np.array_equal(z.real.astype(np.float64), exp.real) and np.array_equal(z.imag.astype(np.float64), exp.imag)


@pytest.mark.parametrize("fmt", [wl.IQ_I16, wl.IQ_F32], ids=["i16", "f32"])
def test_zero_offset_and_one_tap_is_the_discriminator(fmt):
    rng = np.random.default_rng(6093)
    s = rng.integers(-21504, 21505, 5000).astype(np.int16)
    x = iq.fm_modulate(s, sigma=200.0, cfo=0.01, fmt=fmt)
    for gain in (1.0, 5.0 / 3.0):
        assert np.array_equal(_u32(wl.tune(x, [1.0], 1, 0, gain)), _u32(iq.discriminate(x, gain)[0]))


def test_uint8_is_unsigned_around_127_5():
    u = np.stack([np.arange(256), np.arange(256)[::-1]], axis=-1).astype(np.uint8)
    _, z = wl.Tuner([1.0], 1, 0).block(u, want_z=True)
    assert np.array_equal(z.real, np.arange(256) - 127.5) and np.array_equal(z.imag, np.arange(256)[::-1] - 127.5)


def test_the_fma_chains_run_from_tap_0_upwards():
    """acc = fma(h[i], mixed[newest - i], acc) from +0, i = 0, 1, 2: 2^24, then + 1 (lost: a tie to even), then - 2^24 = 0.  From the other end the 1 survives.
    The imaginary chain is independent of the real one: it gets the samples in the other order."""
    big = float(1 << 24)
    mixed = np.array([-big + 1j * big, 1.0 + 1.0j, big - 1j * big], dtype=np.complex64)   # oldest first: tap i meets mixed[2 - i]
    z = wl.fir([1.0, 1.0, 1.0], mixed)
    f32 = np.float32
    up = (f32(big) + f32(1.0)) + f32(-big)
    down = (f32(-big) + f32(1.0)) + f32(big)
    assert up == 0.0 and down == 1.0   # (reordering changes a bit)
    assert z.real == up and z.imag == down
    # fused: h v is not rounded before the add.  (1 + 2^-12)^2 - (1 + 2^-11) = 2^-24 exactly, which a rounded product loses
    a = f32(1.0) + f32(2.0 ** -12)
    z = wl.fir([-1.0, a], np.array([a, f32(1.0) + f32(2.0 ** -11)], dtype=np.complex64))
    assert z.real == 2.0 ** -24 and f32(a * a) - (f32(1.0) + f32(2.0 ** -11)) == 0.0


# ---- 4: end to end on the host form alone ------------------------------------------------------------------------------------------------------------
KINDS = (1, 2, 4)   # stream, packet, packet with FCS
# offsets from the source's centre in Hz: one transmission only 12.5 kHz from its neighbour, all of them inside the +-24 kHz x R the source covers
OFFSETS = {2: (-25000.0, 12500.0, 25000.0), 5: (-75000.0, 12500.0, 25000.0)}
NOISE_SEED = 1


def _good(recs):
    """(LICH records — frame_type 1, cost 0 — do turn up on the bare carrier behind a transmission: the criterion leaves them out)"""
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


@pytest.mark.parametrize("case", [(wl.IQ_I16, 6000.0, 0.0), (wl.IQ_I16, 6000.0, 300.0), (wl.IQ_I16, 6000.0, 1000.0), (wl.IQ_U8, 40.0, 0.0)],
                         ids=["i16_clean", "i16_sigma300", "i16_sigma1000", "u8_clean"])
@pytest.mark.parametrize("R", [2, 5])
def test_three_transmissions_in_one_wideband_carry_their_basebands_frames(basebands, R, case):
    fmt, amplitude, sigma = case
    x = wl.wideband([s for s, _ in basebands], OFFSETS[R], R, amplitude=amplitude, sigma=sigma, seed=NOISE_SEED, fmt=fmt)
    taps = m17hip.wide_default_taps(R)
    for (s, expect), f in zip(basebands, OFFSETS[R]):
        got = _good(fl.demod(wl.tune(x, taps, R, m17hip.wide_fcw(f, R)))[0])
        assert len(expect) >= 7 and got == expect, (R, case, f, len(got), len(expect))


# ---- 4b: the whole operation against a plain float64 statement of it -------------------------------------------------------------------------------------
# wide_lib.tune_f64 on wide_lib.carriers (600 outputs; the default taps at L = 32 R + 1, wide_lib.hamming_taps otherwise): mix at fcw m mod 2^32, filter from a zero history, keep sample n R + R - 1, gain arg(z[n] conj z[n-1]).  The bounds are DERIVED:
#   |z_host - z_f64| <= scale (2^-20.5 + (L + 2) 2^-24), scale = sum|taps| max|x|: the oscillator's asserted 2^-21 on both components (sqrt 2 of it on
#       the complex factor), one rounding of 2^-24 per tap of the fma chain, and two for the cross product that mixes a sample;
#   |y_host - y_f64| (mod 2 pi) <= gain (2 bound / min|z| + 2^-20) wherever z[n] and z[n-1] of the reference both exceed 8 bound: each z is off by at most
#       `bound`, which turns it by at most bound / |z|, and 2^-20 is fm_phase's asserted bound (tests/test_iq_input.py).
# Measured here: the z error reaches at most 0.37 of its bound, the y error 0.13; the reference excludes at most 0.84 % of a case's outputs (cap: 2 %).
F64_RS = (1, 2, 5, 16)
F64_N = 600
F64_GAIN = 1.25
F64_WORDS = {"generic": -0x12345679, "+2^30": 1 << 30, "-2^30": -(1 << 30), "int32_min": -(1 << 31)}
F64_CARRIER_HZ = 0.0   # the carrier's offset from the TUNED word: it is made where the channel listens, whatever the word
F64_EXCLUDED_CAP = 0.02


def _f64_response(taps, R, hz):
    """|H| of the taps at `hz` (at 48000 R samples per second) over sum|taps|."""
    h = np.asarray(taps, dtype=np.float64)
    return abs(np.sum(h * np.exp(-2j * np.pi * hz / (48000.0 * R) * np.arange(h.size)))) / np.abs(h).sum()


def _f64_taps(R, L):
    return m17hip.wide_default_taps(R) if L == 32 * R + 1 else wl.hamming_taps(L)


def _f64_signal(R, fcw, fmt, seed):
    return wl.carriers(R, [fcw], F64_N, fmt, seed, offset_hz=F64_CARRIER_HZ)


_f64_bounds = wl.f64_bound


def _f64_compare(x, taps, R, fcw, what):
    """(z error / its bound, y error / its bound, excluded share) of the host form against the float64 statement; the cap on the excluded share and the
    passband are asserted on the reference alone, before the host form is looked at."""
    L = taps.size
    y64, z64, scale = wl.tune_f64(x, taps, R, fcw, F64_GAIN)
    bound = _f64_bounds(scale, L)
    mag = np.abs(z64)
    ok = np.zeros(F64_N, dtype=bool)
    ok[1:] = (mag[1:] > 8.0 * bound) & (mag[:-1] > 8.0 * bound)
    excluded = 1.0 - ok.mean()
    assert excluded <= F64_EXCLUDED_CAP, (what, excluded)
    assert _f64_response(taps, R, F64_CARRIER_HZ) > 0.5, (what, "the tuned carrier lies inside the passband of these taps")
    lo, hi = (np.int64(fcw) - np.int64(F64_WORDS["generic"])) % (1 << 32), 4294967296.0 / (48000.0 * R)   # (words per Hz)
    if fcw != F64_WORDS["generic"] and 32 * R + 1 == L:
        off = min(lo, (1 << 32) - lo) / hi
        assert _f64_response(taps, R, off) < 0.01, (what, "the generic word's carrier, left in place, would lie outside the default taps' passband")
    y, z = wl.Tuner(taps, R, fcw, F64_GAIN).block(x, want_z=True)
    ez = float(np.abs(z.astype(np.complex128) - z64).max()) / bound
    lowest = np.minimum(mag[1:], mag[:-1])[ok[1:]]
    dy = np.abs(np.angle(np.exp(1j * (y.astype(np.float64) - y64) / F64_GAIN)))[ok] * F64_GAIN
    ey = float((dy / (F64_GAIN * (2.0 * bound / lowest + 2.0 ** -20))).max())
    assert y[0] == 0.0 and y64[0] == 0.0
    return ez, ey, excluded


@pytest.mark.parametrize("fmt", [wl.IQ_I16, wl.IQ_F32], ids=["i16", "f32"])
@pytest.mark.parametrize("R", F64_RS)
def test_the_whole_tuner_is_within_derived_bounds_of_float64(R, fmt):
    worst = [0.0, 0.0, 0.0]
    for L in sorted({1, R, 4 * R + 1, 32 * R + 1, 1024}):
        taps = _f64_taps(R, L)
        assert taps.size == L
        for name, fcw in F64_WORDS.items():
            x = _f64_signal(R, fcw, fmt, seed=6094 + L)
            ez, ey, excluded = _f64_compare(x, taps, R, fcw, (R, L, name))
            assert ez <= 1.0 and ey <= 1.0, (R, L, name, ez, ey)
            worst = [max(a, b) for a, b in zip(worst, (ez, ey, excluded))]
    print(f"tuner vs float64, R = {R}: z error {worst[0]:.3f} of its bound, y error {worst[1]:.3f}, excluded {100 * worst[2]:.2f} %")


def test_a_reference_that_keeps_the_wrong_sample_misses_the_z_bound():
    """The float64 statement with sample n R + R - 2 kept in place of n R + R - 1: the host form is orders of magnitude outside the bound it meets
    against the right one — a tuner with the wrong decimation phase (or a tap shifted by one) could not pass the test above."""
    R = 2
    taps = m17hip.wide_default_taps(R)
    fcw = F64_WORDS["generic"]
    x = _f64_signal(R, fcw, wl.IQ_I16, seed=6094)
    _, z = wl.Tuner(taps, R, fcw, F64_GAIN).block(x, want_z=True)
    _, right, scale = wl.tune_f64(x, taps, R, fcw, F64_GAIN)
    _, shifted, _ = wl.tune_f64(x, taps, R, fcw, F64_GAIN, keep=R - 2)
    bound = _f64_bounds(scale, taps.size)
    assert np.abs(z - right).max() <= bound
    assert np.abs(z - shifted).max() > 1000.0 * bound


# ---- 5: exports and refusals ---------------------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_default_taps", "m17hip_wide_config", "m17hip_wide_channels", "m17hip_upload_wide", "m17hip_upload_wide_device", "m17hip_upload_wide_async",
       "m17hip_upload_wide_device_async"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 609
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for name in ("wide_config", "wide_channels", "upload_wide", "upload_wide_async", "upload_wide_device", "upload_wide_device_async"):
        assert callable(getattr(m17hip.Context, name))
    assert m17hip.IQ_U8 == 3 and m17hip.KERNELS["tune"] == 9
    assert m17hip.wide_fcw(0.0, 5) == 0 and m17hip.wide_fcw(60000.0, 5) == 1 << 30 and m17hip.wide_fcw(-60000.0, 5) == -(1 << 30)
    assert m17hip.wide_fcw(120000.0, 5) == -(1 << 31) and m17hip.wide_fcw(12500.0, 5) == round(12500.0 / 240000.0 * 2 ** 32)


def test_null_context_is_refused_by_every_new_call():
    lib = m17hip.load_library()
    x = np.zeros(640, dtype=np.complex64)
    src, fcw, taps = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.float32)
    assert lib.m17hip_wide_config(C.c_void_p(), C.c_uint32(1), C.c_uint32(5), C.c_int(1), ol._p(taps), C.c_uint32(1)) == -1
    assert lib.m17hip_wide_config(C.c_void_p(), C.c_uint32(1), C.c_uint32(5), C.c_int(1), None, C.c_uint32(0)) == -1
    assert lib.m17hip_wide_channels(C.c_void_p(), ol._p(src), ol._p(fcw), C.c_uint32(1)) == -1
    for name in NEW[3:]:
        assert getattr(lib, name)(C.c_void_p(), ol._p(x), C.c_float(1.0), C.c_uint32(1), C.c_uint32(64), C.c_size_t(640)) == -1, name


def test_python_refuses_what_is_no_wideband_array():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the array is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    for bad in (np.zeros((2, 8), dtype=np.float32), np.zeros((2, 8), dtype=np.complex128), np.zeros((2, 8, 3), dtype=np.int16), np.zeros((2, 8, 2), dtype=np.int8),
                np.zeros((2, 8, 2), dtype=np.uint16), np.zeros(8, dtype=np.uint8)):
        with pytest.raises(TypeError):
            ctx.upload_wide(bad)


@pytest.mark.parametrize("R", [1, 2, 5, 16])
def test_default_taps(R):
    taps = m17hip.wide_default_taps(R)
    assert taps.dtype == np.float32 and taps.size == 32 * R + 1
    assert np.array_equal(taps, taps[::-1]) and abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-6
    assert int(np.argmax(taps)) == 16 * R


def test_default_taps_refusals():
    lib = m17hip.load_library()
    n = C.c_uint32(0)
    buf = np.full(600, 7.0, dtype=np.float32)
    for decim in (0, 17):
        assert lib.m17hip_wide_default_taps(C.c_uint32(decim), ol._p(buf), C.c_uint32(600), C.byref(n)) == -1
    assert lib.m17hip_wide_default_taps(C.c_uint32(5), ol._p(buf), C.c_uint32(160), C.byref(n)) == -1 and n.value == 161   # (too small: the length is still said)
    assert lib.m17hip_wide_default_taps(C.c_uint32(5), None, C.c_uint32(0), C.byref(n)) == -1 and n.value == 161
    assert lib.m17hip_wide_default_taps(C.c_uint32(5), ol._p(buf), C.c_uint32(600), None) == -1
    assert (buf == 7.0).all()
    with pytest.raises(m17hip.M17HipError):
        m17hip.wide_default_taps(17)


# ---- 6: the example, on the host form of the demodulator class ------------------------------------------------------------------------------------------
def test_example_takes_a_wideband_where_it_took_floats(basebands):
    """examples/m17-demod-gpu --wide-i16 / --wide-f32 / --wide-u8 --decim R --offset-hz F [--iq-gain G] on a wideband prints what --float32 prints on the
    host form's floats (M17_DEMOD_DEVICE=cpu: the scalar demodulator; on the GPU path the same class goes through m17hip_upload_wide,
    tests/test_gpu_wide_input.py)."""
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ, M17_DEMOD_DEVICE="cpu")
    R, f = 5, 12500.0
    taps = m17hip.wide_default_taps(R)
    for fmt, flag, amplitude, gain in ((wl.IQ_I16, "--wide-i16", 6000.0, "1"), (wl.IQ_F32, "--wide-f32", 6000.0, "2"), (wl.IQ_U8, "--wide-u8", 40.0, "1")):
        x = wl.wideband([s for s, _ in basebands], OFFSETS[R], R, amplitude=amplitude, sigma=0.0, fmt=fmt)
        y = wl.tune(x, taps, R, m17hip.wide_fcw(f, R), float(gain))
        got = subprocess.run([exe, flag, "--decim", "5", "--offset-hz", "12500", "--iq-gain", gain], input=x.tobytes(), capture_output=True, env=env, check=True).stdout
        exp = subprocess.run([exe, "--float32"], input=y.tobytes(), capture_output=True, env=env, check=True).stdout
        assert got == exp and len(got.splitlines()) >= 6, flag
    assert subprocess.run([exe, "--wide-i16", "--float32"], input=b"", capture_output=True, env=env).returncode == 2
    assert subprocess.run([exe, "--wide-i16", "--decim", "17"], input=b"", capture_output=True, env=env).returncode == 2
    assert subprocess.run([exe, "--wide-u8", "--decim", "5", "--offset-hz", "200000"], input=b"", capture_output=True, env=env).returncode == 2
