"""The HOST form of the wideband signal generator of m17hip_synth_wide (ABI 617): tests/cxx/wide_tx_oracle.cpp — detail/core.h's wtx_index, wtx_step,
wtx_within, wtx_theta, wtx_phase, wtx_add, wtx_noise, wtx_i16 and wtx_u8 under the host compiler — as a feed whose carries go from block to block.
Beside it the definition's integer phase in Python big integers with nothing of core.h in it, a float64 statement of a source's samples from that integer
phase, and the derived bound between the host form's floats and the statement.

TEST INFRASTRUCTURE ONLY, like wide_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

import iq_lib as iq
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "wide_tx_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libwidetxoracle.so")
IQ_I16, IQ_F32, IQ_U8 = wl.IQ_I16, wl.IQ_F32, wl.IQ_U8
TILE = 1024   # csrc/m17_wide_tx_kernels.hpp's WTX_TILE: wideband samples a workgroup makes
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
_lib = None
_p = wl._p


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(iq.CORE)):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        _lib.wt_noise_stream.restype = C.c_uint64
        _lib.wt_unit_noise.restype = C.c_double
        for name in ("wt_theta", "wt_source", "wt_i16", "wt_u8"):
            getattr(_lib, name).restype = None
    return _lib


def k_stated(p, hz_per_unit=None):
    """The deviation word by Python integers / fractions: 2^63 hz / (48000 p^2) rounded half up, hz the exact value of the double (None: 2400 / 21504)."""
    hz = Fraction(2400, 21504) if hz_per_unit is None else Fraction(float(hz_per_unit))
    q = hz * (1 << 63) / (48000 * p * p)
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


def theta(row, P, Q, K, a2=0, last=0, wrong=0):
    """(theta uint64 [W], A2 carry, last sample) of one channel's block by the host form.  wrong: what the definition is NOT (wide_tx_oracle.cpp)."""
    b = np.ascontiguousarray(row, dtype=np.int16)
    assert b.size % Q == 0
    out = np.zeros(b.size // Q * P, dtype=np.uint64)
    c_a2, c_last = C.c_uint64(a2), C.c_int32(last)
    lib().wt_theta(_p(b), C.c_uint32(b.size), C.byref(c_a2), C.byref(c_last), C.c_uint32(P), C.c_uint32(Q), C.c_uint64(K), C.c_int(wrong), _p(out))
    return out, int(c_a2.value), int(c_last.value)


def theta_stated(row, P, Q, K, a2=0, last=0):
    """The same by the definition in Python big integers: k = (m Q) div P, r = (m Q) mod P, A2[k] = A2_carry + sum_{i<k} (b[i-1] + b[i]),
    E = A2[k] P^2 + 2 b[k-1] r P + (b[k] - b[k-1]) r^2, theta = K E mod 2^64.  Returns (list of W ints, the unreduced E as a list, A2 carry, last)."""
    b = [int(last)] + [int(v) for v in row]   # b[i + 1] = sample i
    n = len(b) - 1
    A2 = [int(a2)]
    for i in range(n):
        A2.append(A2[-1] + b[i] + b[i + 1])
    th, Es = [], []
    for m in range(n // Q * P):
        k, r = divmod(m * Q, P)
        E = A2[k] * P * P + 2 * b[k] * r * P + (b[k + 1] - b[k]) * r * r
        Es.append(E)
        th.append((K * E) & M64)
    return th, Es, A2[n] & M64, b[n]


def noise_stream(seed, s):
    return int(lib().wt_noise_stream(C.c_uint64(seed), C.c_uint32(s)))


def quantise(v, fmt):
    """float32 [W][2] -> the block's samples in `fmt`: complex64 [W], int16 or uint8 [W][2]."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if fmt == IQ_F32:
        return v.view(np.complex64).reshape(-1)
    out = np.zeros(v.shape, dtype=np.int16 if fmt == IQ_I16 else np.uint8)
    (lib().wt_i16 if fmt == IQ_I16 else lib().wt_u8)(_p(v), C.c_size_t(v.size), _p(out))
    return out


class Mux:
    """The generator as a feed: sources at 48000 P / Q, a table of (source, fcw, phase0, amplitude) per channel, the channels' carries and the sample count."""

    def __init__(self, sources, P, Q, K, fmt=IQ_I16, sigma=0.0, seed=0, first_sample=0, channels=0):
        self.S, self.P, self.Q, self.K, self.fmt, self.sigma, self.seed = int(sources), int(P), int(Q), int(K), fmt, float(sigma), int(seed)
        self.first = int(first_sample)
        self.table = np.zeros(channels, dtype=[("source", "<u4"), ("fcw", "<i4"), ("phase0", "<u4"), ("amplitude", "<f4")])
        self.reset()

    def reset(self):
        self.count = self.first
        self.a2 = np.zeros(self.table.size, dtype=np.uint64)
        self.last = np.zeros(self.table.size, dtype=np.int32)

    def channels(self, source, fcw, phase0=0, amplitude=0.0):
        n = np.asarray(source).size
        self.table["source"][:n] = source
        self.table["fcw"][:n] = fcw
        self.table["phase0"][:n] = phase0
        self.table["amplitude"][:n] = amplitude

    def floats(self, x, wrong=0):
        """One block of int16 basebands [C][n] -> float32 [S][W][2], the sums before the output format; the carries and the count advance."""
        x = np.ascontiguousarray(x, dtype=np.int16)
        Cn, n = x.shape
        assert Cn <= self.table.size and n % self.Q == 0
        W = n // self.Q * self.P
        out = np.zeros((self.S, W, 2), dtype=np.float32)
        for s in range(self.S):
            # every channel < Cn of the source takes part, amplitude 0 included (a zero term leaves the chain's words as they are): its carries advance
            idx = np.nonzero(self.table["source"][:Cn] == s)[0]
            rows = np.ascontiguousarray(x[idx]) if idx.size else np.zeros((1, n), dtype=np.int16)
            a2 = np.ascontiguousarray(self.a2[idx])
            last = np.ascontiguousarray(self.last[idx])
            fcw = np.ascontiguousarray(self.table["fcw"][idx])
            ph = np.ascontiguousarray(self.table["phase0"][idx])
            amp = np.ascontiguousarray(self.table["amplitude"][idx])
            lib().wt_source(_p(rows), C.c_size_t(n), C.c_uint32(idx.size), C.c_uint32(n), _p(a2), _p(last), _p(fcw), _p(ph), _p(amp), C.c_uint32(self.P),
                            C.c_uint32(self.Q), C.c_uint64(self.K), C.c_uint64(self.count), C.c_float(self.sigma), C.c_uint64(self.seed), C.c_uint32(s),
                            C.c_int(wrong), _p(out[s]))
            self.a2[idx] = a2
            self.last[idx] = last
        self.count += W
        return out

    def block(self, x):
        """One block in the feed's format: complex64 [S][W], int16 or uint8 [S][W][2]."""
        f = self.floats(x)
        return np.stack([quantise(f[s], self.fmt) for s in range(self.S)])


def source_f64(thetas, fcw, phase0, amp, c0):
    """A float64 statement of one source's noiseless samples from the INTEGER phases: thetas[c] the W Python ints (or uint64) of channel c; p = (theta >> 32)
    + fcw M + phase0 mod 2^32 in Python integers, then sum_c amp_c exp(2 pi j p / 2^32) in float64.  Returns (complex128 [W], bound per component):
      the oscillator is within 2^-21 of cos / sin (core.h, asserted in tests/test_wide_input.py over every distinct input; it does not look at the low six
      bits of p, which that figure includes: 2 pi 63 / 2^32 = 9.2e-8 on 2.8e-7), and the product amplitude * cos rounds once, at most 2^-24 of the
      amplitude: amplitude_c (2^-21 + 2^-24) per channel;
      the chain: add j onto a partial sum rounds at most u = 2^-24 of the result, which is at most sum_{i<=j} amplitude_i (1 + 2^-20) in magnitude: the
      adds j = 2 .. n together u (1 + 2^-20) sum_{j>=2} sum_{i<=j} amplitude_i (the first add, onto +0, is exact)."""
    W = len(thetas[0]) if len(thetas) else 0
    z = np.zeros(W, dtype=np.complex128)
    for th, f, p0, a in zip(thetas, fcw, phase0, amp):
        p = np.array([((int(t) >> 32) + int(f) * (int(c0) + m) + int(p0)) & M32 for m, t in enumerate(th)], dtype=np.float64)
        z += float(a) * np.exp(2j * np.pi * p / 4294967296.0)
    amps = [float(a) for a in amp]
    bound = sum(amps) * (2.0 ** -21 + 2.0 ** -24)
    bound += 2.0 ** -24 * (1.0 + 2.0 ** -20) * sum(sum(amps[: j + 1]) for j in range(1, len(amps)))
    return z, bound


def span(P, Q):
    """csrc/m17_wide_tx_kernels.hpp's wtx_span restated: baseband samples a tile can touch."""
    return ((P - 1) + (TILE - 1) * Q) // P + 1
