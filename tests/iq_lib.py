"""The HOST form of the FM discriminator (tests/cxx/iq_oracle.cpp: detail/core.h's fm_cross / fm_phase / fm_discriminate under the host compiler) and
the IQ signals the complex-input tests share.

TEST INFRASTRUCTURE ONLY, like f32_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "iq_oracle.cpp")
CORE = os.path.join(ROOT, "m17-cxx-demod_amd", "include", "m17cxx", "detail", "core.h")
LIB = os.path.join(ROOT, "tests", "cxx", "libiqoracle.so")
IQ_I16, IQ_F32 = 1, 2
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(CORE)):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        for name in ("iqo_discriminate", "iqo_cross", "iqo_phase"):
            getattr(_lib, name).restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fmt_of(row):
    """(format, n, contiguous array) of one row: complex64 [T] or int16 [T][2]."""
    a = np.asarray(row)
    if a.dtype == np.complex64 and a.ndim == 1:
        return IQ_F32, a.size, np.ascontiguousarray(a)
    if a.dtype == np.int16 and a.ndim == 2 and a.shape[1] == 2:
        return IQ_I16, a.shape[0], np.ascontiguousarray(a)
    raise TypeError("a row of IQ is complex64 [T] or int16 [T][2]")


def discriminate(row, gain=1.0, carry=None):
    """(floats[T], carry out) of one row; carry: (i, q) in front of it as floats, None = zero (a fresh feed)."""
    fmt, n, a = fmt_of(row)
    cr = np.zeros(2, dtype=np.float32) if carry is None else np.array(carry, dtype=np.float32)
    out = np.zeros(n, dtype=np.float32)
    lib().iqo_discriminate(_p(a), C.c_int(fmt), C.c_size_t(n), C.c_float(gain), _p(cr), _p(out))
    return out, cr


def discriminate_rows(x, gain=1.0, carry=None):
    """x[C] rows -> (floats[C][T], carries[C][2]); carry: [C][2] or None."""
    outs, crs = [], []
    for c in range(len(x)):
        o, cr = discriminate(x[c], gain, None if carry is None else carry[c])
        outs.append(o)
        crs.append(cr)
    return np.stack(outs), np.stack(crs)


def cross(i, q, pi, pq):
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (i, q, pi, pq)]
    re, im = np.zeros_like(a[0]), np.zeros_like(a[0])
    lib().iqo_cross(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), C.c_size_t(a[0].size), _p(re), _p(im))
    return re, im


def phase(re, im):
    re, im = np.ascontiguousarray(re, dtype=np.float32), np.ascontiguousarray(im, dtype=np.float32)
    out = np.zeros_like(re)
    lib().iqo_phase(_p(re), _p(im), C.c_size_t(re.size), _p(out))
    return out


# ---- the signals ----------------------------------------------------------------------------------------------------------------------------
K_PHASE = (2.0 * np.pi * 2400.0 / 48000.0) / (3.0 * 7168.0)   # radians per sample and int16 unit: the outer symbols (+-3 x 7168) deviate +-2400 Hz
AMPLITUDE = 12000.0


def fm_modulate(s, sigma=0.0, cfo=0.0, fmt=IQ_F32, seed=1, conj=False):
    """IQ of an FM transmitter whose baseband is the int16 row(s) s[..., T]: phase = cumsum(K_PHASE s + cfo), amplitude 12000, complex Gaussian noise
    of `sigma` per component; complex64 [..., T] for IQ_F32, rounded and clipped int16 [..., T][2] for IQ_I16.  conj: the spectrum flipped."""
    s = np.asarray(s)
    ph = np.cumsum(K_PHASE * s.astype(np.float64) + cfo, axis=-1)
    z = AMPLITUDE * np.exp(1j * ph)
    if sigma:
        rng = np.random.default_rng(seed)
        z = z + sigma * (rng.standard_normal(z.shape) + 1j * rng.standard_normal(z.shape))
    if conj:
        z = np.conj(z)
    if fmt == IQ_F32:
        return z.astype(np.complex64)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=-1)), -32768, 32767).astype(np.int16)

