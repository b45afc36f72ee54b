"""CPU-only: wideband IQ input above 16 x in two decimation stages (ABI 610, include/m17hip.h: m17hip_wide_config2, m17hip_wide_default_taps2).  1: pins of
the two-stage HOST form (detail/core.h's ddc_fir2 under the host compiler, tests/cxx/wide2_oracle.cpp) with no polynomial in them — a stage of one tap of 1 and
no decimation leaves the single-stage tuner's words, and the first stage's chains run in tap order.  2: a feed cut anywhere gives the words of the uncut feed,
from counts that cross 2^32.  3: the whole operation against a plain float64 statement of it, within a derived bound, which a wrong decimation phase in either
stage misses.  4: the default first-stage taps do what the header says of them.  5: the feature means something — three FM transmissions in one 2.4 MSPS
source, one of them beyond what any single-stage configuration reaches, carry their basebands' frames.  6: what the new calls promise without a GPU, and the
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
import wide2_lib as w2
import wide_lib as wl

LICH = 1
FORMATS = {"i16": wl.IQ_I16, "f32": wl.IQ_F32, "u8": wl.IQ_U8}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _noise(fmt, W, seed):
    rng = np.random.default_rng(seed)
    if fmt == wl.IQ_I16:
        return rng.integers(-20000, 20001, size=(W, 2)).astype(np.int16)
    if fmt == wl.IQ_U8:
        return rng.integers(0, 256, size=(W, 2)).astype(np.uint8)
    return (rng.standard_normal(W) + 1j * rng.standard_normal(W)).astype(np.complex64) * np.float32(3000.0)


# ---- 1: pins without a polynomial -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_a_first_stage_of_one_tap_and_no_decimation_leaves_the_single_stage_tuner(fmt):
    R2, L2 = 5, 41
    x = _noise(fmt, 400 * R2, 6101)
    taps2 = wl.hamming_taps(L2)
    fcw = m17hip.wide_fcw(31000.0, R2)
    assert np.array_equal(_u32(w2.tune2(x, [1.0], 1, taps2, R2, fcw, 1.25)), _u32(wl.tune(x, taps2, R2, fcw, 1.25)))


@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_a_second_stage_of_one_tap_and_no_decimation_leaves_the_single_stage_tuner(fmt):
    R1, L1 = 6, 29
    x = _noise(fmt, 400 * R1, 6102)
    taps1 = wl.hamming_taps(L1)
    fcw = m17hip.wide_fcw(-52000.0, R1)
    assert np.array_equal(_u32(w2.tune2(x, taps1, R1, [1.0], 1, fcw, 1.25)), _u32(wl.tune(x, taps1, R1, fcw, 1.25)))


def test_the_first_stage_chains_run_from_tap_0_upwards():
    """Stage 1 of three taps of 1 over mixed = x (fcw = 0: the oscillator is exactly (1, 0)), stage 2 one tap of 1: u = fma(h[i], mixed[2 - i], u) from +0,
    i = 0, 1, 2: 2^24, then + 1 (lost: a tie to even), then - 2^24 = 0.  From the other end the 1 survives; the imaginary chain gets the samples in the
    other order, so one output shows both."""
    big = float(1 << 24)
    x = np.array([-big + 1j * big, 1.0 + 1.0j, big - 1j * big], dtype=np.complex64)   # oldest first: tap i meets x[2 - i]
    _, z = w2.Tuner2([1.0, 1.0, 1.0], 3, [1.0], 1, 0).block(x, want_z=True)
    f32 = np.float32
    up = (f32(big) + f32(1.0)) + f32(-big)
    down = (f32(-big) + f32(1.0)) + f32(big)
    assert up == 0.0 and down == 1.0   # (reordering changes a word)
    assert z.size == 1 and z[0].real == up and z[0].imag == down
    # ... and so do the second stage's over the u: one tap of 1 in stage 1, no decimation there
    _, z = w2.Tuner2([1.0], 1, [1.0, 1.0, 1.0], 3, 0).block(x, want_z=True)
    assert z.size == 1 and z[0].real == up and z[0].imag == down


# ---- 2: the feed ----------------------------------------------------------------------------------------------------------------------------------------
PH_T, PH_R1, PH_R2, PH_L1, PH_L2 = 3000, 3, 2, 7, 25
PH_CUTS = np.cumsum([0, 1, 2, 255, 1024]).tolist() + [PH_T]


@pytest.fixture(scope="module")
def ph_case():
    rng = np.random.default_rng(6103)
    x = rng.integers(-20000, 20001, size=(PH_T * PH_R1 * PH_R2, 2)).astype(np.int16)
    taps1 = rng.standard_normal(PH_L1).astype(np.float32) / np.float32(PH_L1)
    taps2 = rng.standard_normal(PH_L2).astype(np.float32) / np.float32(PH_L2)
    x.setflags(write=False)
    return x, taps1, taps2


@pytest.mark.parametrize("start", [0, (1 << 32) + 12345, (1 << 32) - 700], ids=["zero", "above_2^32", "across_2^32"])
def test_a_two_stage_feed_cut_at_block_boundaries_gives_the_words_of_the_uncut_feed(ph_case, start):
    x, taps1, taps2 = ph_case
    R = PH_R1 * PH_R2
    fcw = m17hip.wide_fcw(31000.0, R)
    whole = w2.Tuner2(taps1, PH_R1, taps2, PH_R2, fcw, 1.25, count=start).block(x)
    t = w2.Tuner2(taps1, PH_R1, taps2, PH_R2, fcw, 1.25, count=start)
    parts = [t.block(x[a * R: b * R]) for a, b in zip(PH_CUTS[:-1], PH_CUTS[1:])]
    assert np.array_equal(_u32(np.concatenate(parts)), _u32(whole))
    # ... and the count matters: the same blocks from another count are other words
    other = w2.Tuner2(taps1, PH_R1, taps2, PH_R2, fcw, 1.25, count=start + 1).block(x)
    assert not np.array_equal(_u32(other), _u32(whole))


# ---- 3: against float64 ---------------------------------------------------------------------------------------------------------------------------------
# wide2_lib.tune2_f64 on wide_lib.carriers (600 outputs), wide_lib.hamming_taps in both stages.  The bounds are DERIVED (wide2_lib.f64_bound2's docstring):
#   |z_host - z_f64| <= scale (2^-20.5 + (L1 + L2 + 2) 2^-24), scale = sum|taps2| sum|taps1| max|x|;
#   |y_host - y_f64| (mod 2 pi) <= gain (2 bound / min|z| + 2^-20) wherever z[n] and z[n-1] of the reference both exceed 8 bound (wide_lib.f64_check_y's rule).
# At most 1 % of a case's outputs may fall under that floor: asserted on the float64 reference alone, before the host form is looked at.
# The last two are the configurations tests/test_gpu_wide2_input.py launches with fewer than 64 u per chain of a chunk (Q = 56 and Q = 45).
F64_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (10, 5, 81, 161), (16, 1, 129, 33), (3, 16, 1, 513), (16, 16, 256, 1024), (16, 12, 256, 1024), (16, 16, 256, 700)]
F64_N = 600
F64_GAIN = 1.25
F64_WORDS = {"generic": -0x12345679, "+2^30": 1 << 30, "int32_min": -(1 << 31)}
F64_EXCLUDED_CAP = 0.01


@pytest.mark.parametrize("fmt", [wl.IQ_I16, wl.IQ_F32], ids=["i16", "f32"])
@pytest.mark.parametrize("case", F64_CASES, ids=[f"{a}x{b}_{c}_{d}" for a, b, c, d in F64_CASES])
def test_the_two_stage_tuner_is_within_derived_bounds_of_float64(case, fmt):
    R1, R2, L1, L2 = case
    taps1, taps2 = wl.hamming_taps(L1), wl.hamming_taps(L2)
    worst = [0.0, 0.0, 0.0]
    for name, fcw in F64_WORDS.items():
        x = wl.carriers(R1 * R2, [fcw], F64_N, fmt, seed=6104 + L2)
        y64, z64, scale = w2.tune2_f64(x, taps1, R1, taps2, R2, fcw, F64_GAIN)
        bound = w2.f64_bound2(scale, L1, L2)
        excluded = 1.0 - float(w2.f64_ok(z64, bound).mean())
        assert excluded <= F64_EXCLUDED_CAP, (case, name, excluded)
        y, z = w2.Tuner2(taps1, R1, taps2, R2, fcw, F64_GAIN).block(x, want_z=True)
        ez, ey, _ = w2.f64_errors(y, z, y64, z64, bound, F64_GAIN)
        assert y[0] == 0.0 and y64[0] == 0.0
        assert ez <= 1.0 and ey <= 1.0, (case, name, ez, ey)
        worst = [max(a, b) for a, b in zip(worst, (ez, ey, excluded))]
    print(f"two stages vs float64, {case}: z error {worst[0]:.3f} of its bound, y error {worst[1]:.3f}, excluded {100 * worst[2]:.2f} %")


def test_the_restated_lds_layout_gives_the_recorded_q_and_bytes():
    """wide2_lib.q_and_lds against the table NOTES.md recorded for ABI 610 and the two configurations added since: the GPU cases that are there for Q < 64
    do have Q < 64, and none asks for more than 64 KB."""
    table = {(10, 5, 81, 161): (64, 34688), (2, 3, 5, 7): (64, 12368), (16, 1, 129, 33): (64, 38144), (3, 16, 1, 513): (64, 45056),
             (16, 16, 256, 1024): (40, 65280)}
    for (R1, R2, L1, L2), e in table.items():
        assert w2.q_and_lds(L1, R1, L2, R2) == e, (R1, R2, L1, L2)
    assert w2.q_and_lds(256, 16, 1024, 12)[0] == 56 and w2.q_and_lds(256, 16, 700, 16)[0] == 45
    for R1 in range(1, 17):
        for R2 in range(1, 17):
            q, lds = w2.q_and_lds(256, R1, 1024, R2)
            assert 40 <= q <= 64 and lds <= 65536, (R1, R2, q, lds)


def test_a_wrong_decimation_phase_in_either_stage_misses_the_z_bound():
    """The float64 statement with sample p R1 + R1 - 2 kept by stage 1, or u n R2 + R2 - 2 kept by stage 2, in place of the last of each group: the host form
    is far outside the bound it meets against the right one."""
    R1, R2, L1, L2 = 10, 5, 81, 161
    taps1, taps2 = wl.hamming_taps(L1), wl.hamming_taps(L2)
    fcw = F64_WORDS["generic"]
    x = wl.carriers(R1 * R2, [fcw], F64_N, wl.IQ_I16, seed=6104)
    _, z = w2.Tuner2(taps1, R1, taps2, R2, fcw, F64_GAIN).block(x, want_z=True)
    _, right, scale = w2.tune2_f64(x, taps1, R1, taps2, R2, fcw, F64_GAIN)
    _, first, _ = w2.tune2_f64(x, taps1, R1, taps2, R2, fcw, F64_GAIN, keep1=R1 - 2)
    _, second, _ = w2.tune2_f64(x, taps1, R1, taps2, R2, fcw, F64_GAIN, keep2=R2 - 2)
    bound = w2.f64_bound2(scale, L1, L2)
    e = [float(np.abs(z - r).max()) / bound for r in (right, first, second)]
    print(f"z error over its bound: right {e[0]:.3f}, stage 1 one sample early {e[1]:.1f}, stage 2 one sample early {e[2]:.1f}")
    assert e[0] <= 1.0
    assert e[1] > 1.0 and e[2] > 1.0


# ---- 4: the default taps --------------------------------------------------------------------------------------------------------------------------------
PASS_DB, STOP_DB = 0.01, -65.0   # (measured in float64 for every pair: within 0.003 dB and at least 69 dB down)


@pytest.mark.parametrize("R1", range(2, 17))
def test_default_first_stage_taps(R1):
    worst_pass, worst_stop = 0.0, -1000.0
    for R2 in range(2, 17):
        taps1, taps2 = m17hip.wide_default_taps2(R1, R2)
        assert taps1.dtype == np.float32 and taps1.size == 8 * R1 + 1
        assert abs(float(taps1.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(taps2, m17hip.wide_default_taps(R2))
        rate = 48000.0 * R1 * R2
        p = np.abs(w2.response_db(taps1, rate, np.linspace(-6000.0, 6000.0, 241))).max()
        # the bands the first decimation folds onto the channel: k * 48000 * R2 +- 12 kHz, k = 1 .. R1 - 1 (the taps are real: the negative k mirror them)
        hz = np.concatenate([k * 48000.0 * R2 + np.linspace(-12000.0, 12000.0, 97) for k in range(1, R1)])
        s = w2.response_db(taps1, rate, hz).max()
        assert p <= PASS_DB and s <= STOP_DB, (R1, R2, p, s)
        worst_pass, worst_stop = max(worst_pass, p), max(worst_stop, s)
    print(f"default stage-1 taps, decim1 = {R1}: passband within {worst_pass:.4f} dB, alias bands at most {worst_stop:.1f} dB")


def test_default_taps_of_a_first_stage_that_does_not_decimate():
    for R2 in (1, 5, 16):
        taps1, taps2 = m17hip.wide_default_taps2(1, R2)
        assert taps1.tolist() == [1.0] and np.array_equal(taps2, m17hip.wide_default_taps(R2))


# ---- 5: end to end at 2.4 MSPS on the host form alone ---------------------------------------------------------------------------------------------------
KINDS = (1, 2, 4)   # stream, packet, packet with FCS
R1, R2 = 10, 5
# offsets from the source's centre in Hz: one transmission only 12.5 kHz from its neighbour, one beyond the +-384 kHz the widest single-stage source covers
# (and beyond +-600 kHz), all inside the +-1.2 MHz this source covers
OFFSETS = (-762500.0, 12500.0, 25000.0)
# the existing test's sigma 300 at R = 5 is a noise density of 300^2 / 240 kHz per component; the same density at 2.4 MSPS is 300 sqrt(10)
SIGMA = 300.0 * np.sqrt(10.0)
CLIPPED_CAP = 0.001
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


@pytest.mark.parametrize("case", [(wl.IQ_I16, 6000.0, 0.0), (wl.IQ_I16, 6000.0, SIGMA), (wl.IQ_U8, 40.0, 0.0)], ids=["i16_clean", "i16_noise", "u8_clean"])
def test_three_transmissions_in_one_2400k_source_carry_their_basebands_frames(basebands, case):
    fmt, amplitude, sigma = case
    assert all(abs(f) <= 24000.0 * R1 * R2 for f in OFFSETS) and max(abs(f) for f in OFFSETS) > 600000.0
    x = wl.wideband([s for s, _ in basebands], OFFSETS, R1 * R2, amplitude=amplitude, sigma=sigma, seed=NOISE_SEED, fmt=fmt)
    rails = (-32768, 32767) if fmt == wl.IQ_I16 else (0, 255)
    clipped = float(((x == rails[0]) | (x == rails[1])).any(axis=-1).mean())   # (a sample ON a rail counts as clipped: an upper bound)
    print(f"{case}: {100 * clipped:.4f} % of the samples on a rail")
    assert clipped <= CLIPPED_CAP, clipped
    taps1, taps2 = m17hip.wide_default_taps2(R1, R2)
    for (s, expect), f in zip(basebands, OFFSETS):
        got = _good(fl.demod(w2.tune2(x, taps1, R1, taps2, R2, m17hip.wide_fcw(f, R1 * R2)))[0])
        assert len(expect) >= 7 and got == expect, (case, f, len(got), len(expect))


# ---- 6: exports, refusals, the Python layer and the example ---------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_default_taps2", "m17hip_wide_config2"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 610
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_config2) and callable(m17hip.wide_default_taps2)
    assert m17hip.KERNELS["tune2"] == 10 and m17hip.KERNELS["tune"] == 9
    assert m17hip.wide_fcw(600000.0, 50) == 1 << 30 and m17hip.wide_fcw(-1200000.0, 50) == -(1 << 31)


def _defaults2(d1, d2, t1, c1, n1, t2, c2, n2):
    return m17hip.load_library().m17hip_wide_default_taps2(C.c_uint32(d1), C.c_uint32(d2), t1, C.c_uint32(c1), n1, t2, C.c_uint32(c2), n2)


def test_default_taps2_refusals():
    n1, n2 = C.c_uint32(0), C.c_uint32(0)
    b1, b2 = np.full(200, 7.0, dtype=np.float32), np.full(600, 7.0, dtype=np.float32)
    p1, p2 = ol._p(b1), ol._p(b2)
    for d1, d2 in ((0, 5), (17, 5), (10, 0), (10, 17)):
        assert _defaults2(d1, d2, p1, 200, C.byref(n1), p2, 600, C.byref(n2)) == -1, (d1, d2)
    for d1, d2 in ((1, 1), (16, 16), (1, 16), (16, 1)):   # (the limits themselves are served)
        assert _defaults2(d1, d2, p1, 200, C.byref(n1), p2, 600, C.byref(n2)) == 0, (d1, d2)
        assert (n1.value, n2.value) == (1 if d1 == 1 else 8 * d1 + 1, 32 * d2 + 1)
    b1[:], b2[:] = 7.0, 7.0
    assert _defaults2(10, 5, p1, 80, C.byref(n1), p2, 600, C.byref(n2)) == -1 and (n1.value, n2.value) == (81, 161)   # (too small: the lengths are still said)
    assert _defaults2(10, 5, p1, 200, C.byref(n1), p2, 160, C.byref(n2)) == -1 and (n1.value, n2.value) == (81, 161)
    assert _defaults2(10, 5, None, 0, C.byref(n1), None, 0, C.byref(n2)) == -1 and (n1.value, n2.value) == (81, 161)
    assert _defaults2(10, 5, None, 200, C.byref(n1), p2, 600, C.byref(n2)) == -1
    assert _defaults2(10, 5, p1, 200, C.byref(n1), None, 600, C.byref(n2)) == -1
    assert _defaults2(10, 5, p1, 200, None, p2, 600, C.byref(n2)) == -1
    assert _defaults2(10, 5, p1, 200, C.byref(n1), p2, 600, None) == -1
    assert (b1 == 7.0).all() and (b2 == 7.0).all()   # (nothing written by a refused call)
    assert _defaults2(10, 5, p1, 81, C.byref(n1), p2, 161, C.byref(n2)) == 0 and (b1[81:] == 7.0).all() and (b2[161:] == 7.0).all()
    for bad in ((0, 5), (10, 17)):
        with pytest.raises(m17hip.M17HipError):
            m17hip.wide_default_taps2(*bad)


def test_null_context_is_refused_by_wide_config2():
    lib = m17hip.load_library()
    taps = np.ones(1, dtype=np.float32)
    args = (C.c_uint32(1), C.c_uint32(10), ol._p(taps), C.c_uint32(1), C.c_uint32(5), ol._p(taps), C.c_uint32(1), C.c_int(1))
    assert lib.m17hip_wide_config2(C.c_void_p(), *args) == -1
    assert lib.m17hip_wide_config2(C.c_void_p(), C.c_uint32(1), C.c_uint32(10), None, C.c_uint32(0), C.c_uint32(5), None, C.c_uint32(0), C.c_int(1)) == -1


def test_python_refuses_a_block_that_does_not_fit_the_two_stage_configuration():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the array is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    ctx._wide = (2, 50, m17hip.IQ_I16)   # what wide_config2(2, 10, 5) leaves: rows are multiples of 50 samples
    for bad in (np.zeros((2, 40, 2), dtype=np.int16), np.zeros((2, 99, 2), dtype=np.int16), np.zeros((1, 100, 2), dtype=np.int16),
                np.zeros((2, 100, 2), dtype=np.uint8), np.zeros((2, 100), dtype=np.complex64), np.zeros((2, 100, 2), dtype=np.float32)):
        with pytest.raises(TypeError):
            ctx.upload_wide(bad)


def test_example_takes_a_2400k_source_in_two_stages(basebands):
    """examples/m17-demod-gpu --wide-i16 / --wide-u8 --decim 10 --decim2 5 --offset-hz F on a 2.4 MSPS source prints what --float32 prints on the host
    form's floats (M17_DEMOD_DEVICE=cpu: the scalar demodulator, which keeps the u between outputs where the host form of the tests recomputes them; on
    the GPU path the same class goes through m17hip_wide_config2, tests/test_gpu_wide2_input.py)."""
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ, M17_DEMOD_DEVICE="cpu")
    taps1, taps2 = m17hip.wide_default_taps2(R1, R2)
    for fmt, flag, amplitude, gain, f in ((wl.IQ_I16, "--wide-i16", 6000.0, "1", OFFSETS[1]), (wl.IQ_U8, "--wide-u8", 40.0, "2", OFFSETS[0])):
        x = wl.wideband([s for s, _ in basebands], OFFSETS, R1 * R2, amplitude=amplitude, sigma=0.0, fmt=fmt)
        y = w2.tune2(x, taps1, R1, taps2, R2, m17hip.wide_fcw(f, R1 * R2), float(gain))
        got = subprocess.run([exe, flag, "--decim", "10", "--decim2", "5", "--offset-hz", str(int(f)), "--iq-gain", gain], input=x.tobytes(),
                             capture_output=True, env=env, check=True).stdout
        exp = subprocess.run([exe, "--float32"], input=y.tobytes(), capture_output=True, env=env, check=True).stdout
        assert got == exp and len(got.splitlines()) >= 6, flag
    assert subprocess.run([exe, "--wide-i16", "--decim", "10", "--decim2", "17"], input=b"", capture_output=True, env=env).returncode == 2
    assert subprocess.run([exe, "--wide-i16", "--decim", "10", "--decim2", "0"], input=b"", capture_output=True, env=env).returncode == 2
    assert subprocess.run([exe, "--wide-u8", "--decim", "10", "--decim2", "5", "--offset-hz", "1300000"], input=b"", capture_output=True, env=env).returncode == 2
