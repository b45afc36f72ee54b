"""The HOST form of the tuner of m17hip_upload_wide (tests/cxx/wide_oracle.cpp: detail/core.h's nco / ddc_mix / ddc_tap / ddc_fir under the host compiler,
with iq_lib's discriminator behind them) and the wideband signals the tests share.

TEST INFRASTRUCTURE ONLY, like iq_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq

ROOT = iq.ROOT
SRC = os.path.join(ROOT, "tests", "cxx", "wide_oracle.cpp")
LIB = os.path.join(ROOT, "tests", "cxx", "libwideoracle.so")
IQ_I16, IQ_F32, IQ_U8 = 1, 2, 3
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(iq.CORE)):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        for name in ("wo_nco", "wo_fir", "wo_tune"):
            getattr(_lib, name).restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def nco(p):
    """(cos, sin) as float32 arrays of the phases p (uint32)."""
    p = np.ascontiguousarray(p, dtype=np.uint32)
    c, s = np.zeros(p.shape, dtype=np.float32), np.zeros(p.shape, dtype=np.float32)
    lib().wo_nco(_p(p), C.c_size_t(p.size), _p(c), _p(s))
    return c, s


def fir(h, mixed):
    """The filter's sum over len(h) mixed samples (complex64, oldest first): one complex64."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    m = np.ascontiguousarray(mixed, dtype=np.complex64)
    assert m.size == h.size
    z = np.zeros(1, dtype=np.complex64)
    lib().wo_fir(_p(h), C.c_uint32(h.size), _p(m), _p(z))
    return z[0]


def fmt_of(row):
    """(format, samples, contiguous array) of one source row: complex64 [W], int16 or uint8 [W][2]."""
    a = np.asarray(row)
    if a.dtype == np.complex64 and a.ndim == 1:
        return IQ_F32, a.size, np.ascontiguousarray(a)
    if a.dtype in (np.int16, np.uint8) and a.ndim == 2 and a.shape[1] == 2:
        return (IQ_I16 if a.dtype == np.int16 else IQ_U8), a.shape[0], np.ascontiguousarray(a)
    raise TypeError("a source row is complex64 [W], or int16 / uint8 [W][2]")


class Tuner:
    """One channel on one source, as a feed: the source's history, the sample count and the channel's carry go from block to block."""

    def __init__(self, taps, decim, fcw, gain=1.0, count=0):
        self.h = np.ascontiguousarray(taps, dtype=np.float32)
        self.R, self.fcw, self.gain, self.count = int(decim), int(fcw), float(gain), int(count)
        self.hist = np.zeros((max(self.h.size - 1, 1), 2), dtype=np.float32)
        self.carry = np.zeros(2, dtype=np.float32)

    def block(self, row, want_z=False):
        fmt, W, a = fmt_of(row)
        assert W % self.R == 0
        n = W // self.R
        out = np.zeros(n, dtype=np.float32)
        z = np.zeros(n, dtype=np.complex64) if want_z else None
        lib().wo_tune(_p(a), C.c_int(fmt), C.c_size_t(n), C.c_uint32(self.R), _p(self.h), C.c_uint32(self.h.size), C.c_int32(self.fcw), C.c_uint64(self.count),
                      _p(self.hist), _p(self.carry), C.c_float(self.gain), _p(out), None if z is None else _p(z))
        self.count += W
        return (out, z) if want_z else out


def tune(row, taps, decim, fcw, gain=1.0):
    """The floats of one whole feed in one block."""
    return Tuner(taps, decim, fcw, gain).block(row)


def tune_f64(row, taps, decim, fcw, gain=1.0, keep=None):
    """The whole operation stated in float64, with nothing of detail/core.h in it: x[m] exp(-2 pi j ((fcw m) mod 2^32) / 2^32), z[n] = sum_i taps[i]
    mixed[n R + R - 1 - i] from a zero history, y[n] = gain arg(z[n] conj z[n-1]) with y[0] = 0.  Returns (y, z, scale = sum|taps| max|x|: what one
    unit of relative error in a product is worth in z).  `keep` (default R - 1) is the sample of each group of R that is kept: a test hands in
    another one to show that a wrong decimation phase misses its bound."""
    fmt, W, a = fmt_of(row)
    R = int(decim)
    assert W % R == 0
    if fmt == IQ_F32:
        x = a.astype(np.complex128)
    else:
        x = a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64) - ((127.5 + 127.5j) if fmt == IQ_U8 else 0.0)
    m = np.arange(W, dtype=np.uint64)
    p = (m * np.uint64(int(fcw) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)   # (m < 2^32: the product fits 64 bits)
    mixed = x * np.exp(-2j * np.pi * (p.astype(np.float64) / 4294967296.0))
    h = np.asarray(taps, dtype=np.float64).reshape(-1)
    z = np.convolve(mixed, h)[:W][(R - 1 if keep is None else int(keep))::R]
    y = np.zeros(z.size, dtype=np.float64)
    y[1:] = gain * np.angle(z[1:] * np.conj(z[:-1]))
    return y, z, float(np.abs(h).sum() * np.abs(x).max())


def f64_bound(scale, L):
    """|z - z_f64| of float32 arithmetic in the tuner's order: the oscillator's asserted 2^-21 on both components (sqrt 2 of it on the complex factor), one
    rounding of 2^-24 per tap of the fma chain and two for the cross product that mixes a sample, each on a term of at most `scale`."""
    return scale * (2.0 ** -20.5 + (L + 2) * 2.0 ** -24)


def f64_check_y(y, x, taps, decim, fcw, gain):
    """Floats y of one channel against tune_f64: (the largest |y - y_f64| mod 2 pi gain over ITS bound gain (2 bound / min|z| + 2^-20), the share of
    outputs the bound does not speak about: z[n] or z[n-1] of the reference at or below 8 bound).  2^-20 is fm_phase's asserted bound."""
    y64, z64, scale = tune_f64(x, taps, decim, fcw, gain)
    bound = f64_bound(scale, np.asarray(taps).size)
    mag = np.abs(z64)
    ok = np.zeros(mag.size, dtype=bool)
    ok[1:] = (mag[1:] > 8.0 * bound) & (mag[:-1] > 8.0 * bound)
    lowest = np.minimum(mag[1:], mag[:-1])[ok[1:]]
    dy = np.abs(np.angle(np.exp(1j * (np.asarray(y, dtype=np.float64) - y64) / gain)))[ok] * gain
    return float((dy / (gain * (2.0 * bound / lowest + 2.0 ** -20))).max()), 1.0 - float(ok.mean())


def hamming_taps(L):
    """A Hamming window of unit DC gain, its peak a third of a tap off the middle: a low-pass all of whose taps are positive and no two equal (not the two
    in the middle of an even length either: a swap of any two neighbours shows), so that z grows from the first output on even where a short block never
    fills the filter (a windowed sinc's first outputs are its side lobes' partial sums, below the magnitude the phase bound needs) and a dropped or shifted
    tap changes every output."""
    t = np.arange(L, dtype=np.float64) - 0.5 * (L - 1) - 1.0 / 3.0
    h = 0.54 + 0.46 * np.cos(2.0 * np.pi * t / (L + 1))
    return (h / h.sum()).astype(np.float32)


def carriers(decim, words, n, fmt, seed, offset_hz=0.0):
    """One source row of n outputs: per frequency word a carrier of amplitude 6000 `offset_hz` off the word (so inside the passband of a channel tuned to
    it, whatever the word), each with a slow phase modulation; noise of sigma 100 per component."""
    R = int(decim)
    W = n * R
    m = np.arange(W, dtype=np.int64)
    z = np.zeros(W, dtype=np.complex128)
    for i, fcw in enumerate(words):
        turns = ((m * (int(fcw) & 0xFFFFFFFF)) % (1 << 32)).astype(np.float64) / 4294967296.0 + offset_hz / (48000.0 * R) * m
        z += 6000.0 * np.exp(1j * (2.0 * np.pi * turns + 0.8 * np.sin(2.0 * np.pi * m / (300.0 * R) + i)))
    rng = np.random.default_rng(seed)
    z = z + 100.0 * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    if fmt == IQ_F32:
        return z.astype(np.complex64)
    if fmt == IQ_U8:
        return np.clip(np.rint(np.stack([z.real, z.imag], axis=-1) / 128.0 + 127.5), 0, 255).astype(np.uint8)
    return np.rint(np.stack([z.real, z.imag], axis=-1)).astype(np.int16)


class Feeds:
    """One host-form tuner per channel, fed block by block over data[S] (whole source rows); retuning is writing src[c] / fcw[c] (a channel's carry
    goes with it, the history and the count are the source's)."""

    def __init__(self, data, taps, src, fcw, decim, gain):
        self.data, self.taps, self.R, self.gain = data, taps, int(decim), float(gain)
        self.per_source = [Tuner(taps, decim, 0, gain) for _ in range(len(data))]   # (for the histories and the count alone)
        self.src, self.fcw = list(src), list(fcw)
        self.carry = [np.zeros(2, dtype=np.float32) for _ in src]

    def block(self, a, b):
        out = []
        for c in range(len(self.src)):
            s = self.src[c]
            t = Tuner(self.taps, self.R, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            out.append(t.block(self.data[s][a * self.R: b * self.R]))
            self.carry[c] = t.carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][a * self.R: b * self.R])
        return np.stack(out)


def tune_channels(x, source, fcw, taps, decim, gain=1.0):
    """x[S] source rows, one block of a fresh feed -> floats [C][W / decim] for channels (source[c], fcw[c])."""
    return np.stack([tune(x[s], taps, decim, w, gain) for s, w in zip(source, fcw)])


# ---- the signals ----------------------------------------------------------------------------------------------------------------------------
def wideband(basebands, offsets_hz, decim, amplitude=6000.0, sigma=0.0, seed=1, fmt=IQ_I16):
    """One source row holding an FM transmission per int16 baseband row (iq_lib's deviation), each linearly interpolated to decim x and put at its
    offset from the centre; complex Gaussian noise of `sigma` per component.  int16 [W][2] (rounded, clipped), complex64 [W] or — around 127.5 — uint8."""
    R = int(decim)
    n = min(len(b) for b in basebands)
    W = n * R
    m = np.arange(W, dtype=np.float64)
    z = np.zeros(W, dtype=np.complex128)
    for b, f in zip(basebands, offsets_hz):
        s = np.interp(m / R, np.arange(n, dtype=np.float64), np.asarray(b[:n], dtype=np.float64))
        ph = np.cumsum(iq.K_PHASE / R * s) + 2.0 * np.pi * f / (48000.0 * R) * m
        z += amplitude * np.exp(1j * ph)
    if sigma:
        rng = np.random.default_rng(seed)
        z = z + sigma * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    if fmt == IQ_F32:
        return z.astype(np.complex64)
    v = np.stack([z.real, z.imag], axis=-1)
    if fmt == IQ_I16:
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return np.clip(np.rint(v + 127.5), 0, 255).astype(np.uint8)
