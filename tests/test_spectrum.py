"""CPU-only: the source spectrum (ABI 616, include/m17hip.h: m17hip_wide_spectrum, m17hip_wide_spectrum_default_window, m17hip_wide_spectrum_twiddles,
m17hip_wide_spectrum_fetch).  1: the twiddle table and the default window against their formulas in double.  2: exports, version, the refusals of the
context-free calls.  3: the frame rule against a brute-force statement in Python integers, across 2^32 and 2^40.  4: the two-stage pass a device may take
gives the radix-2 stages' words.  5: the HOST form (tests/spectrum_lib.py: detail/core.h under the host compiler) against np.fft.fft in float64 within a
derived bound that a frame start, a window index or a bin order off by one misses; the single chain is told from the two-level sum by its words.  6: a feed
cut into blocks.  7: wide_spectrum_carriers, and the workflow it is for — survey, pick, assign, demodulate — on the three transmissions of
tests/test_resample_input.py's 2.048 MSPS source."""
import ctypes as C

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as sp
import survey_lib as sl
import test_resample_input as tri

POINTS = (64, 128, 256, 512, 1024, 2048, 4096)
U = 2.0 ** -24


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ramp(N):
    """A window a caller supplies: a ramp from 0.25 to 1.25, so that a frame or a window index off by one sample shows (a stationary tone under a smooth
    window would hide it)."""
    return (0.25 + np.arange(N) / N).astype(np.float32)


# ---- 1: the data ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", POINTS)
def test_twiddles_and_default_window_are_their_formulas_in_double(N):
    tw = m17hip.wide_spectrum_twiddles(N)
    assert tw.shape == (N // 2,) and tw.dtype == np.complex64
    j = np.arange(N // 2)
    exact = np.exp(-2j * np.pi * j / N)
    assert float(np.abs(tw.real.astype(np.float64) - exact.real).max()) <= U and float(np.abs(tw.imag.astype(np.float64) - exact.imag).max()) <= U
    # exactly on the axes, zeroes included
    assert _u32(tw[:1].view(np.float32)).tolist() == _u32([1.0, 0.0]).tolist()
    assert tw[N // 4].real == 0.0 and tw[N // 4].imag == -1.0
    # tw[N / 2 - j] = (-re, im) of tw[j], to the bit
    lo, hi = tw[1: N // 4], tw[N // 2 - 1: N // 4: -1]
    assert np.array_equal(_u32(hi.real), _u32(-lo.real)) and np.array_equal(_u32(hi.imag), _u32(lo.imag))
    w = m17hip.wide_spectrum_default_window(N)
    assert w.shape == (N,) and w.dtype == np.float32
    x = 2.0 * np.pi * np.arange(N) / N
    stated = 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)
    assert float(np.abs(w.astype(np.float64) - stated).max()) <= U   # (all values are at most 1: half an ulp of the rounding and the doubles' own error)
    assert abs(float(w[N // 2]) - 1.0) <= U and 0.0 < float(w[0]) < 1e-4 and np.isfinite(w).all()


# ---- 2: exports, refusals ---------------------------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_spectrum", "m17hip_wide_spectrum_default_window", "m17hip_wide_spectrum_twiddles", "m17hip_wide_spectrum_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 616
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert m17hip.KERNELS["spectrum"] == 14 and m17hip.KERNELS["resample"] == 13
    for f in (m17hip.wide_spectrum_default_window, m17hip.wide_spectrum_twiddles, m17hip.wide_spectrum_carriers, m17hip.Context.wide_spectrum,
              m17hip.Context.wide_spectrum_fetch):
        assert callable(f)
    assert sp.frames_per_pass_and_lds(4096) == (1, 49152) and sp.frames_per_pass_and_lds(64) == (16, 8448) and sp.frames_per_pass_and_lds(256)[0] == 8


def test_the_context_free_calls_refuse_and_write_nothing():
    lib = m17hip.load_library()
    for f in (lib.m17hip_wide_spectrum_default_window, lib.m17hip_wide_spectrum_twiddles):
        buf = np.full(4096, 7.0, dtype=np.float32)
        for points in (0, 1, 32, 63, 65, 96, 1000, 8192, 1 << 31):
            assert f(C.c_uint32(points), ol._p(buf), C.c_uint32(buf.size)) == -1, points
        assert f(C.c_uint32(64), None, C.c_uint32(64)) == -1 and f(C.c_uint32(64), ol._p(buf), C.c_uint32(63)) == -1
        assert (buf == 7.0).all()
        assert f(C.c_uint32(64), ol._p(buf), C.c_uint32(64)) == 0 and (buf[64:] == 7.0).all() and not (buf[:64] == 7.0).any()
    with pytest.raises(m17hip.M17HipError):
        m17hip.wide_spectrum_twiddles(100)
    with pytest.raises(m17hip.M17HipError):
        m17hip.wide_spectrum_default_window(32)
    # a NULL context
    w = np.ones(64, dtype=np.float32)
    assert lib.m17hip_wide_spectrum(C.c_void_p(), C.c_uint32(64), C.c_uint32(64), ol._p(w), C.c_uint32(64)) == -1
    assert lib.m17hip_wide_spectrum_fetch(C.c_void_p(), C.c_uint32(0), ol._p(w), C.c_uint64(64), None, None) == -1


# ---- 3: the frame rule ------------------------------------------------------------------------------------------------------------------------------------
def test_the_frame_rule_is_the_brute_force_statement_across_2_32_and_2_40():
    N = 64
    seen = set()
    for hop in (1, 3000, N):
        for c0 in (0, hop - 1, hop, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7):
            for W in (0, 1, N - 1, N, N + 1, N + hop - 1, N + hop, 3 * hop + N + 5, 7001):
                got, stated = sp.frames(c0, W, N, hop), sp.frames_stated(c0, W, N, hop)
                assert got == stated, (hop, c0, W, got, stated)
                first, J = got
                assert first == (hop - c0 % hop) % hop and (c0 + first) % hop == 0
                assert J == 0 or first + (J - 1) * hop + N <= W < first + J * hop + N
                seen.add(J)
    assert {0, 1, 2, 4} <= seen
    # 32 bits of the count are not enough: 2^32 + 1 and 1 give different firsts at a hop that does not divide 2^32
    assert sp.frames(2 ** 32 + 1, 7001, N, 3000)[0] != sp.frames(1, 7001, N, 3000)[0]
    # at the ABI's limits
    assert sp.frames(2 ** 64 - 1, 2 ** 32 - 1, 4096, 1 << 24) == sp.frames_stated(2 ** 64 - 1, 0, 4096, 1 << 24)[:1] + ((2 ** 32 - 1 - 4096 - 1) // (1 << 24) + 1,)


# ---- 4: two stages in one pass ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", POINTS)
def test_two_stages_in_one_pass_give_the_radix_2_words(N):
    """core::spec_item2 (what the kernel runs: stage 1 alone where log2 N is odd, then pairs of stages) against core::spec_item1 stage by stage: equal
    words, on noise and on a frame with an infinity and a NaN in it; and the radix-2 form is a DFT."""
    rng = np.random.default_rng(6160 + N)
    v = (1000.0 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    a, b = sp.fft(v), sp.fft(v, fused=True)
    assert np.array_equal(_u32(a.view(np.float32)), _u32(b.view(np.float32)))
    ref = np.fft.fft(v.astype(np.complex128))
    n = N.bit_length() - 1
    assert float(np.abs(a - ref).max()) <= 5 * n * U * float(np.abs(v).sum()) * (1 + 2.0 ** -10)   # (spectrum_lib.plane_f64's bound without the window)
    bad = v.copy()
    bad[3], bad[N // 2 + 1] = np.inf, complex(np.nan, 1.0)
    a, b = sp.fft(bad).view(np.float32), sp.fft(bad, fused=True).view(np.float32)
    assert not np.isfinite(a).any()   # (it reaches every bin of its frame)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_u32(a)[~np.isnan(a)], _u32(b)[~np.isnan(b)])


# ---- 5: against float64 -----------------------------------------------------------------------------------------------------------------------------------
def _noise_block(N, J, hop, rng, extra=5):
    W = (J - 1) * hop + N + extra
    return rng.integers(-20000, 20001, size=(W, 2)).astype(np.int16)


@pytest.mark.parametrize("N", (64, 1024, 4096))
def test_the_host_form_is_np_fft_within_a_derived_bound_that_mistakes_miss(N):
    """White noise, a ramp window, hop N / 2 + 3 (overlapping frames, an odd start), J = 1, 16, 17, 40 frames: the host form lies within
    spectrum_lib.plane_f64's bound of sum_f |np.fft.fft(w x_f)|^2, the two-stage pass gives the same plane, and a frame start off by one sample, a window
    index off by one and a mirrored bin order each miss the bound at least tenfold (measured: the host form within 0.0125 of the bound at every size; the
    mistakes between 44 and 7.6e5 times it)."""
    rng = np.random.default_rng(6161 + N)
    w, hop = _ramp(N), N // 2 + 3
    worst = 0.0
    for J in (1, 16, 17, 40):
        x = _noise_block(N, J, hop, rng)
        P, j, first = sp.plane(x, N, hop, w)
        P64, B, J64, first64 = sp.plane_f64(x, N, hop, w)
        assert (j, first) == (J, 0) == (J64, first64) and (B > 0).all()
        ratio = lambda Q: float((np.abs(np.asarray(Q, dtype=np.float64) - P64) / B).max())
        worst = max(worst, ratio(P))
        assert np.array_equal(_u32(sp.plane(x, N, hop, w, fused=True)[0]), _u32(P))
        wrong = {"frame start + 1": ratio(sp.plane(x, N, hop, w, shift=1)[0]), "window index + 1": ratio(sp.plane(x, N, hop, w, wshift=1)[0]),
                 "mirrored bins": ratio(P[(-np.arange(N)) % N])}
        print(f"spectrum vs float64, N {N} J {J}: {ratio(P):.4f} of its bound; " + ", ".join(f"{k} {v:.1f}" for k, v in wrong.items()))
        assert ratio(P) <= 1.0, (N, J)
        for k, v in wrong.items():
            assert v >= 10.0, (N, J, k, v)
    print(f"spectrum vs float64, N {N}: largest ratio {worst:.4f}")


def test_the_two_level_sum_is_not_the_single_chain():
    """A single-level sum cannot be told from the definition by a float64 bound: it IS an accurate sum, and lies as far inside the bound as the two-level
    one (measured 0.02 of it at J = 40 against 0.009) — the bound has to hold the FFT's roundings, thousands of times what the order of a few adds moves.
    What pins the order is the words: up to 17 frames the two levels ARE the single chain (a second group of one power adds the same number), at 40 they
    are not — on this data 42 of 64 bins differ."""
    N, hop = 64, 35
    rng = np.random.default_rng(6162)
    w = _ramp(N)
    differs = {}
    for J in (1, 16, 17, 40):
        x = _noise_block(N, J, hop, rng)
        two, one = sp.plane(x, N, hop, w)[0], sp.plane(x, N, hop, w, single=True)[0]
        P64, B, _, _ = sp.plane_f64(x, N, hop, w)
        assert float((np.abs(one.astype(np.float64) - P64) / B).max()) <= 1.0
        differs[J] = int((_u32(two) != _u32(one)).sum())
    print(f"bins of {N} whose two-level sum differs from the single chain: {differs}")
    assert differs[1] == 0 and differs[16] == 0 and differs[17] == 0
    assert differs[40] > 0, "the test data does not tell the two-level sum from a single chain"


def test_no_frame_gives_a_plane_of_positive_zeroes_and_the_default_window_is_taken():
    x = np.ones((63, 2), dtype=np.int16)
    P, J, first = sp.plane(x, 64, 1)
    assert J == 0 and first == 0 and (_u32(P) == 0).all()
    # the default window on a tone at bin 5 of 64: the power stands in bins 3..7 (a four-term window's main lobe), 90 dB over the rest
    n = np.arange(640)
    t = np.exp(2j * np.pi * 5 * n / 64)
    x = np.stack([np.rint(8000 * t.real), np.rint(8000 * t.imag)], axis=-1).astype(np.int16)
    P, J, _ = sp.plane(x, 64, 64)
    assert J == 10 and int(np.argmax(P)) == 5
    assert float(P[[0, 1, 9, 10, 32, 59, 63]].max()) < 1e-8 * float(P[5])


# ---- 6: the feed ------------------------------------------------------------------------------------------------------------------------------------------
def test_frames_follow_the_feeds_count_not_the_blocks():
    """A feed cut into ragged blocks: every block's first frame starts where the FEED's index is a multiple of hop; a block whose frames all lie inside one
    block of the uncut feed's grid holds the same frames, so a cut at a multiple of hop loses only the frames that straddle it."""
    N, hop = 64, 48
    rng = np.random.default_rng(6163)
    x = rng.integers(-3000, 3001, size=(1, 1000, 2)).astype(np.int16)
    cuts = [0, 1, 50, 63 + 50, 400, 401, 1000]
    got = sp.planes(x, N, hop, cuts)
    for (a, b), (plane, J, first_sample) in zip(zip(cuts[:-1], cuts[1:]), got):
        starts = [m for m in range(a, b - N + 1) if m % hop == 0]
        assert J == len(starts) and first_sample % hop == 0 and first_sample >= a
        if starts:
            assert first_sample == starts[0]
            alone = sp.plane(x[0][starts[0]: starts[-1] + N], N, hop, None, starts[0])   # (the same frames as a block of their own)
            assert alone[1] == J and np.array_equal(_u32(alone[0]), _u32(plane[0]))
        else:
            assert (_u32(plane) == 0).all()
    assert [g[1] for g in got] == [0, 0, 0, 5, 0, 11]


# ---- 7: carriers ------------------------------------------------------------------------------------------------------------------------------------------
def test_carriers_of_a_stated_plane():
    """Two carriers 12.5 kHz apart and one across the wrap, on a flat floor: found at their centroids, strongest first, with their dB over the floor; a
    carrier's shoulders are not carriers; a row with a zero or non-finite median reports nothing."""
    N, rate = 2048, 2048000.0
    p = np.full((4, N), 2.0)
    hz = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N) * (rate / N)

    def carrier(row, f, power):   # a Gaussian of 2 kHz sigma: shoulders over the floor beyond the 4.5 kHz half band
        d = (hz - f + rate / 2) % rate - rate / 2
        row += power * np.exp(-0.5 * (d / 2000.0) ** 2)

    carrier(p[1], 12500.0, 4e4)
    carrier(p[1], 25250.0, 1e4)
    carrier(p[1], -1023000.0, 2e3)
    p[2, : N // 2 + 1] = 0.0   # (median 0)
    carrier(p[2], -300000.0, 4e4)
    p[3, : N // 2 + 1] = np.inf   # (median not finite)
    found = m17hip.wide_spectrum_carriers(p.astype(np.float32), rate)
    assert [s for s, _, _ in found] == [1, 1, 1]
    assert all(abs(f - t) < 100.0 for (_, f, _), t in zip(found, (12500.0, 25250.0, -1023000.0))), found
    assert found[0][2] > found[1][2] > found[2][2] > 10.0 and all(-rate / 2 <= f < rate / 2 for _, f, _ in found)
    assert m17hip.wide_spectrum_carriers(p[0], rate) == [] and m17hip.wide_spectrum_carriers(p[2:], rate) == []
    assert len(m17hip.wide_spectrum_carriers(p[1], rate, margin_db=35.0)) == 1


# How far a tuner may be off: measured on the host form of the resampling tuner and the float oracle (NOTES.md, ABI 616) — each of the three transmissions
# tuned at its true offset +- e keeps all 7 of 7 records for e up to 900 Hz (100 Hz steps to 800, then 850, 900; 950 Hz loses records on the + side).
TUNE_E = 900.0
# N = 2048 (1 kHz bins: nine to a 9 kHz band) over the whole source as one block, hop = N: the float64 statement ALONE finds the three within 60 Hz
# (asserted below within TUNE_E / 2 before the host form is looked at).
CAR_N = 2048


def test_the_spectrum_finds_the_three_transmissions_and_the_tuner_decodes_them_at_the_found_offsets():
    """Survey, pick, assign, demodulate on tests/test_resample_input.py's 2.048 MSPS int16 source (its transmissions stand at -762.5, +12.5 and +25 kHz):
    wide_spectrum_carriers on the host-form plane finds exactly three, each within TUNE_E / 2 of a true offset, and the host resampler tuned at the FOUND
    offsets decodes each transmission's frames."""
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tri.KINDS]
    x = tri.source_2048k(bb)
    rate = 2048000.0
    w = m17hip.wide_spectrum_default_window(CAR_N)
    P64, B, J, _ = sp.plane_f64(x, CAR_N, CAR_N, w)
    stated = m17hip.wide_spectrum_carriers(P64, rate)
    assert len(stated) == 3
    for f in tri.OFFSETS:
        assert min(abs(hz - f) for _, hz, _ in stated) <= TUNE_E / 2, (f, stated)
    P, Jh, first = sp.plane(x, CAR_N, CAR_N, w)
    assert (Jh, first) == (J, 0) and J == x.shape[0] // CAR_N
    assert float((np.abs(P.astype(np.float64) - P64) / B).max()) <= 1.0
    found = m17hip.wide_spectrum_carriers(P, rate)
    print("carriers:", [(s, round(hz, 1), round(db, 1)) for s, hz, db in found])
    assert len(found) == 3 and all(s == 0 and db > 30.0 for s, _, db in found), found
    taps1, taps2 = m17hip.wide_resample_default_taps(tri.CH_R1, tri.CH_U, tri.CH_D)
    for s, f in zip(bb, tri.OFFSETS):
        hz = min((hz for _, hz, _ in found), key=lambda h: abs(h - f))
        assert abs(hz - f) <= TUNE_E / 2, (f, hz)
        expect = tri._good(ol.demod(s)[0])
        y = rl.resample(x, taps1, tri.CH_R1, tri.CH_U, tri.CH_D, taps2, m17hip.wide_fcw(hz, rate / 48000.0))
        got = tri._good(fl.demod(y)[0])
        assert len(got) == 7 and [p for _, p in got] == [p for _, p in expect], (f, hz, len(got), len(expect))
