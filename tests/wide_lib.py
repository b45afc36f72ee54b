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
