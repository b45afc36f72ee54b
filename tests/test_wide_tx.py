"""CPU-only: the wideband signal generator (ABI 617, include/m17hip.h: m17hip_synth_wide_k, m17hip_synth_wide_config, m17hip_synth_wide_channels,
m17hip_synth_wide).  1: the deviation word against Python integers / fractions, and its refusals.  2: version, exports and bindings.  3: the HOST form's
integer phase (detail/core.h's wtx_* under the host compiler, tests/cxx/wide_tx_oracle.cpp) against the definition in Python big integers.  4: a feed cut
raggedly gives the bytes of the uncut feed.  5: the host form's floats within a derived bound of a float64 statement from the same integer phase — which an
off-by-one in k, r taken from m instead of m Q, or the undelayed baseband each miss many-fold.  6: the phase means the deviation it says: theta / 2^64
against a float64 trapezoid of the interpolated baseband.  7: the noise and the output formats.  8: a loopback on the host — three transmissions multiplexed
at 2.048 MSPS and received by the resampling tuner's host form carry their basebands' frames."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import wide_tx_lib as wt

RATES = [(1, 1), (5, 1), (128, 3), (625, 12)]


def _k(hz, p):
    k = C.c_uint64(0)
    code = m17hip.load_library().m17hip_synth_wide_k(C.c_double(hz), C.c_uint32(p), C.byref(k))
    return code, int(k.value)


def _rows(rng, n, Q):
    """Basebands with +-32768-scale steps: full-scale alternation, a random walk of large steps, plain noise."""
    n = n // Q * Q
    alt = np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    rnd = rng.integers(-32768, 32768, n).astype(np.int16)
    slow = np.clip(np.cumsum(rng.integers(-3000, 3001, n)), -32768, 32767).astype(np.int16)
    return [alt, rnd, slow]


# ---- 1: the deviation word ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 5, 50, 128, 2000])
def test_the_deviation_word_is_the_rounded_quotient(p):
    assert _k(0.0, p) == (0, wt.k_stated(p)) and m17hip.synth_wide_k(0.0, p) == wt.k_stated(p)
    assert wt.k_stated(p) == ((1 << 63) + 215040 * p * p) // (430080 * p * p)   # 2400 / 21504 / 48000 = 1 / 430080
    for hz in (0.1, 1.0 / 3.0, 2400.0 / 21504.0, 7.5e-4 * p, 3.0 * p * p):
        assert _k(hz, p) == (0, wt.k_stated(p, hz)), (hz, p)


def test_the_deviation_word_refusals():
    lib = m17hip.load_library()
    k = C.c_uint64(77)
    for hz, p in ((0.0, 0), (0.0, 2001), (-1.0, 5), (float("nan"), 5), (float("inf"), 5), (48000.0, 1), (1e30, 5), (1e-30, 5), (5e-324, 2000)):
        assert lib.m17hip_synth_wide_k(C.c_double(hz), C.c_uint32(p), C.byref(k)) == -1 and k.value == 77, (hz, p)
    assert lib.m17hip_synth_wide_k(C.c_double(0.0), C.c_uint32(5), None) == -1
    assert _k(47999.0, 1)[0] == 0   # (just below half a turn per unit of E)
    with pytest.raises(m17hip.M17HipError):
        m17hip.synth_wide_k(0.0, 0)


# ---- 2: exports and bindings ------------------------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_synth_wide_k", "m17hip_synth_wide_config", "m17hip_synth_wide_channels", "m17hip_synth_wide", "m17hip_synth_wide_device"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 617
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for name in ("synth_wide_config", "synth_wide_channels", "synth_wide"):
        assert callable(getattr(m17hip.Context, name)), name
    assert callable(m17hip.synth_wide_k) and m17hip.KERNELS["synth_wide"] == 15 and m17hip.KERNELS["spectrum"] == 14
    assert m17hip.WIDE_TX_DTYPE.itemsize == 16 and m17hip.WIDE_TX_DTYPE.names == ("source", "fcw", "phase0", "amplitude")


def test_null_contexts_and_pointers_are_refused():
    lib = m17hip.load_library()
    buf = np.zeros(64, dtype=np.int16)
    tx = np.zeros(1, dtype=m17hip.WIDE_TX_DTYPE)
    assert lib.m17hip_synth_wide_config(None, C.c_uint32(1), C.c_uint32(5), C.c_uint32(1), C.c_int(1), C.c_uint64(1), C.c_float(0), C.c_uint64(0), C.c_uint64(0)) == -1
    assert lib.m17hip_synth_wide_channels(None, tx.ctypes.data_as(C.c_void_p), C.c_uint32(1)) == -1
    for name in ("m17hip_synth_wide", "m17hip_synth_wide_device"):
        assert getattr(lib, name)(None, buf.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.c_uint32(4), C.c_size_t(16)) == -1
    assert not buf.any()


# ---- 3: the integer phase ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "{}_{}".format(*r))
def test_the_host_forms_phase_is_the_definitions_in_big_integers(rate):
    P, Q = rate
    rng = np.random.default_rng(100 * P + Q)
    K = wt.k_stated(P)
    n = max(2400 // P, 4) * Q
    for i, row in enumerate(_rows(rng, n, Q)):
        a2, last = int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(-32768, 32768))
        for k_word in (K, int(rng.integers(1, 1 << 62)) * 2 + 1):   # (the configured word, and one that wraps theta at every step)
            got, a2n, lastn = wt.theta(row, P, Q, k_word, a2, last)
            exp, _, a2e, laste = wt.theta_stated(row, P, Q, k_word, a2, last)
            assert got.size == row.size // Q * P and [int(v) for v in got] == exp, (rate, i)
            assert (a2n, lastn) == (a2e, laste)


# ---- 4: feed invariance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [wt.IQ_I16, wt.IQ_F32, wt.IQ_U8], ids=["i16", "f32", "u8"])
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "{}_{}".format(*r))
def test_a_feed_cut_raggedly_gives_the_bytes_of_the_uncut_feed(rate, fmt):
    P, Q = rate
    rng = np.random.default_rng(7 * P + Q)
    groups = [1, 2, 7, 1, 13, 2, 5]   # blocks of Q, 2 Q and prime multiples of Q
    n = sum(groups) * Q
    x = np.stack(_rows(rng, n, Q))
    first = 3 * P

    def feed():
        m = wt.Mux(2, P, Q, wt.k_stated(P), fmt, sigma=40.0, seed=5, first_sample=first, channels=3)
        m.channels([0, 1, 0], [123456789, -987654321, 55555], [1, 2, 3 << 30], [900.0, 2000.0, 700.0])
        return m
    whole = feed().block(x)
    m, parts, a = feed(), [], 0
    for g in groups:
        parts.append(m.block(x[:, a: a + g * Q]))
        a += g * Q
    assert [p.shape[1] for p in parts] == [g * P for g in groups]
    assert np.concatenate(parts, axis=1).tobytes() == whole.tobytes()
    other = wt.Mux(2, P, Q, wt.k_stated(P), fmt, sigma=40.0, seed=5, first_sample=first + P, channels=3)
    other.channels([0, 1, 0], [123456789, -987654321, 55555], [1, 2, 3 << 30], [900.0, 2000.0, 700.0])
    assert other.block(x).tobytes() != whole.tobytes()   # (the count matters)


# ---- 5: the floats against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "{}_{}".format(*r))
def test_the_floats_are_within_the_derived_bound_of_float64_and_mistakes_are_not(rate):
    P, Q = rate
    rng = np.random.default_rng(31 * P + Q)
    K = wt.k_stated(P)
    n = max(1800 // P, 6) * Q
    x = np.stack(_rows(rng, n, Q) + [rng.integers(-20000, 20001, n // Q * Q).astype(np.int16)])
    fcw = [int(v) for v in rng.integers(-(1 << 31), 1 << 31, 4)]
    ph0 = [int(v) for v in rng.integers(0, 1 << 32, 4)]
    amp = [3000.0, 1.0, 7777.5, 12000.0]
    c0 = 5 * P

    def floats(wrong):
        m = wt.Mux(1, P, Q, K, wt.IQ_F32, first_sample=c0, channels=4)
        m.channels([0] * 4, fcw, ph0, amp)
        return m.floats(x, wrong)[0].astype(np.float64)
    th = [wt.theta_stated(row, P, Q, K)[0] for row in x]
    z, bound = wt.source_f64(th, fcw, ph0, amp, c0)

    def ratio(v):
        return float(max(np.abs(v[:, 0] - z.real).max(), np.abs(v[:, 1] - z.imag).max()) / bound)
    r = ratio(floats(0))
    print(f"P / Q = {P} / {Q}: worst error {r:.3f} of the bound {bound:.3e}")
    assert r <= 1.0
    for wrong, what in ((1, "k one too small"), (2, "r from m instead of m Q"), (3, "the undelayed baseband")):
        if wrong == 2 and Q == 1:
            continue   # (m Q is m)
        rw = ratio(floats(wrong))
        print(f"    {what}: {rw:.1f} of the bound")
        assert rw > 100.0, (what, rw)


# ---- 6: the physical deviation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [(5, 1), (128, 3), (625, 12), (2000, 1)], ids=lambda r: "{}_{}".format(*r))
def test_the_phase_is_the_integral_of_the_interpolated_baseband_at_the_deviation(rate):
    """theta / 2^64 turns, unwrapped (K E / 2^64 from the unreduced E), against hz / 48000 * the integral over time, in baseband samples, of the baseband
    interpolated linearly from b[k-1] to b[k] — a float64 trapezoid.  Bound: K is the exact quotient rounded to an integer, off by at most 1/2, which moves
    K E / 2^64 by at most |E| / 2^65; the float64 statement's own rounding, below 8 n 2^-53 of hz / 48000 * sum |b|."""
    P, Q = rate
    hz = Fraction(2400, 21504)
    K = m17hip.synth_wide_k(0.0, P)
    rng = np.random.default_rng(P)
    n = max(3000 // P, 4) * Q
    b = np.clip(np.cumsum(rng.integers(-4000, 4001, n)), -32768, 32767).astype(np.int16)
    _, E, _, _ = wt.theta_stated(b, P, Q, K)
    turns = np.array([float(Fraction(K * e, 1 << 64)) for e in E])
    bb = np.concatenate([[0.0], b.astype(np.float64)])   # bb[k] = b[k - 1]
    area = np.concatenate([[0.0], np.cumsum((bb[:-1] + bb[1:]) / 2.0)])   # the integral up to baseband sample k
    m = np.arange(len(E))
    k, r = (m * Q) // P, ((m * Q) % P) / float(P)
    stated = float(hz) / 48000.0 * (area[k] + bb[k] * r + (bb[k + 1] - bb[k]) * r * r / 2.0)
    bound = max(abs(e) for e in E) / 2.0 ** 65 + 8 * n * 2.0 ** -53 * float(hz) / 48000.0 * float(np.abs(b.astype(np.float64)).sum())
    worst = float(np.abs(turns - stated).max())
    print(f"P / Q = {P} / {Q}: worst {worst:.3e} turns, {worst / bound:.3f} of the bound {bound:.3e}")
    assert worst <= bound
    # a symbol of +3 x 7168 held for a second deviates +2400 Hz: 2400 turns
    _, Es, _, _ = wt.theta_stated(np.full(2 * Q, 21504, dtype=np.int16), P, Q, K, a2=0, last=21504)
    assert Es[1] - Es[0] == 2 * 21504 * P * Q   # (E grows by 2 b P per unit of m Q: 2 b P^2 per baseband sample)
    per_second = Fraction(K * 2 * 21504 * P * P, 1 << 64) * 48000
    assert abs(float(per_second) - 2400.0) <= 2400.0 * 0.5 / K * 1.001


# ---- 7: noise and output formats ----------------------------------------------------------------------------------------------------------------------------
def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & wt.M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & wt.M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & wt.M64
    return x ^ (x >> 31)


def _unit_noise(stream, n):
    h = _splitmix(stream ^ ((n * 0xD1342543DE82EF95) & wt.M64))
    g = _splitmix(h)
    total = sum((h >> (16 * k)) & 0xFFFF for k in range(4)) + sum((g >> (16 * k)) & 0xFFFF for k in range(4))
    return float(2 * total - 8 * 65535) * 0.5 * (1.0 / 53510.38419625641)


def test_the_noise_is_the_modulators_from_all_64_bits_of_the_count():
    lib = wt.lib()
    for seed, s in ((0, 0), (5, 1), ((1 << 64) - 1, 255)):
        ns = _splitmix(seed ^ _splitmix((s * 0x9E3779B97F4A7C15 + 0x57494445) & wt.M64))
        assert wt.noise_stream(seed, s) == ns
        for n in (0, 1, 2, (1 << 33) - 1, (1 << 33) + 2, (1 << 64) - 1):
            assert lib.wt_unit_noise(C.c_uint64(ns), C.c_uint64(n)) == _unit_noise(ns, n)
    # a silent source with noise: the words at count M are unit_noise(ns, 2 M) and (ns, 2 M + 1) times sigma, rounded to float
    c0 = (1 << 32) - 4
    m = wt.Mux(2, 1, 1, wt.k_stated(1), wt.IQ_F32, sigma=250.0, seed=9, first_sample=c0, channels=1)
    v = m.floats(np.zeros((1, 8), dtype=np.int16))
    for s in range(2):
        ns = wt.noise_stream(9, s)
        exp = [[np.float32(_unit_noise(ns, 2 * (c0 + i)) * 250.0), np.float32(_unit_noise(ns, 2 * (c0 + i) + 1) * 250.0)] for i in range(8)]
        assert v[s].tobytes() == np.array(exp, dtype=np.float32).tobytes()


def test_the_output_formats_round_to_even_and_clamp():
    v = np.array([0.5, 1.5, -0.5, -1.5, 2.5000002, 32766.5, 32767.5, 1e9, -32768.5, -1e9, 64.0, -64.0, 16320.0, 16384.0, -16320.0, -16448.0, 63.9, np.inf, -np.inf],
                 dtype=np.float32)
    assert list(wt.quantise(v.reshape(1, -1), wt.IQ_I16)[0]) == [0, 2, 0, -2, 3, 32766, 32767, 32767, -32768, -32768, 64, -64, 16320, 16384, -16320, -16448, 64,
                                                                  32767, -32768]
    # uint8: v / 128 + 127.5 in one fma, then to even: 64 -> 128, -64 -> 127, 16320 -> 255, -16320 -> 0
    assert list(wt.quantise(v.reshape(1, -1), wt.IQ_U8)[0]) == [128, 128, 127, 127, 128, 255, 255, 255, 0, 0, 128, 127, 255, 255, 0, 0, 128, 255, 0]
    assert wt.quantise(v[:4].reshape(2, 2), wt.IQ_F32).tobytes() == v[:4].tobytes()


def test_a_term_of_amplitude_0_leaves_the_words_as_they_are():
    rng = np.random.default_rng(3)
    x = np.stack(_rows(rng, 40, 1))
    a = wt.Mux(1, 5, 1, wt.k_stated(5), wt.IQ_F32, channels=3)
    a.channels([0, 0, 0], [1 << 30, 77, -(1 << 29)], 0, [500.0, 0.0, 300.0])
    b = wt.Mux(1, 5, 1, wt.k_stated(5), wt.IQ_F32, channels=2)
    b.channels([0, 0], [1 << 30, -(1 << 29)], 0, [500.0, 300.0])
    assert a.block(x).tobytes() == b.block(x[[0, 2]]).tobytes()
    silent = wt.Mux(2, 5, 1, wt.k_stated(5), wt.IQ_F32, channels=3)
    assert silent.block(x).tobytes() == np.zeros((2, 200), dtype=np.complex64).tobytes()   # (+0, not -0)


# ---- 8: loopback on the host --------------------------------------------------------------------------------------------------------------------------------
from test_resample_input import CH_D, CH_R1, CH_U, KINDS, OFFSETS, SIGMA, _good   # noqa: E402  (that test's transmissions and its criterion)


def test_three_transmissions_multiplexed_at_2048k_carry_their_basebands_frames():
    """The three transmissions of tests/test_resample_input.py — same kinds, offsets and ol.generate parameters —, multiplexed by the host form at
    2.048 MSPS (P / Q = 128 / 3) as int16 with that test's noise, received by resample_lib's host-form tuner and the float oracle: that test's own criterion.
    The generator delays every baseband by one sample (it interpolates from b[k - 1] to b[k]); the demodulator finds its own symbol clock, so the records'
    payloads need no account of it."""
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in KINDS]
    n = min(b.size for b in bb) // CH_U * CH_U
    P, Q = CH_R1 * CH_D, CH_U
    assert 48000 * P == 2048000 * Q
    A = 8000.0
    assert len(bb) * A + 8.0 * SIGMA <= 32767.0
    m = wt.Mux(1, P, Q, m17hip.synth_wide_k(0.0, P), wt.IQ_I16, sigma=SIGMA, seed=1, channels=3)
    m.channels([0, 0, 0], [m17hip.wide_fcw(f, P / Q) for f in OFFSETS], 0, A)
    x = m.block(np.stack([b[:n] for b in bb]))[0]
    assert x.shape == (n // Q * P, 2) and int(x.max()) < 32767 and int(x.min()) > -32768   # no sample clips
    taps1, taps2 = m17hip.wide_resample_default_taps(CH_R1, CH_U, CH_D)
    for s, f in zip(bb, OFFSETS):
        expect = _good(ol.demod(s)[0])
        y = rl.resample(x, taps1, CH_R1, CH_U, CH_D, taps2, m17hip.wide_fcw(f, P / Q))
        got = _good(fl.demod(y)[0])
        print(f"{f} Hz: {len(got)} records")
        assert len(got) == 7 and [p for _, p in got] == [p for _, p in expect], (f, len(got), len(expect))
