"""The HOST form of the channeliser of m17hip_wide_raster (tests/cxx/raster_oracle.cpp: detail/core.h's chan_fold / chan_pass1 / chan_pass2 under the host
compiler, the discriminator behind them), its float64 statement with nothing of core.h in it, the derived bound and the kernel's tile size restated.
wide_lib and wide2_lib are imported as they stand: their signals and their float64 rules for y are used here.

TEST INFRASTRUCTURE ONLY, like wide_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import m17hip
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "raster_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "librasteroracle.so")
_lib = None
_p = wl._p
# (M, decim, taps) where indexing can go wrong: 6 = 3 x 2 with 7 and 13 taps at decim 4; M = 12 with 5 taps, so seven residues get no tap; decim = M;
# decim > M; gcd(decim, M) = 1.  The CPU and the GPU tests share them.
SMALL = [(6, 4, 7), (6, 4, 13), (12, 4, 5), (8, 8, 20), (6, 9, 20), (9, 4, 30)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(iq.CORE)):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
    return _lib


def factor(M):
    """(M1, M2) as the library factors M, or None where it refuses it."""
    m1, m2 = C.c_uint32(0), C.c_uint32(0)
    return (m1.value, m2.value) if lib().ro_factor(C.c_uint32(M), C.byref(m1), C.byref(m2)) else None


def factor_stated(M):
    """The rule of detail/core.h's chan_factor in words of its own: M2 the largest divisor of M with M2^2 <= M, M1 = M / M2, accepted when M1 <= 16."""
    if not 1 <= M <= 256:
        return None
    m2 = max(d for d in range(1, M + 1) if M % d == 0 and d * d <= M)
    return (M // m2, m2) if M // m2 <= 16 else None


def tile_and_lds(L, R, M):
    """csrc/m17_chan_kernels.hpp's chan_tile and chan_lds_bytes restated: (outputs per tile, LDS bytes of a workgroup).  In float2: TT R + L samples, M
    twiddles and two planes of TT + 1 rows of M | 1 (an odd pitch); TT the largest that fits 64 KB, 31 at the most."""
    mp = M | 1
    tt = min((65536 // 8 - L - M - 2 * mp) // (R + 2 * mp), 31)
    return tt, 8 * (tt * R + L + M + 2 * (tt + 1) * mp)


def twiddles_f64(M):
    """exp(-2 pi j k / M) in float64."""
    return np.exp(-2j * np.pi * np.arange(M, dtype=np.float64) / M)


class Raster:
    """Channels on ONE source, as a feed: the source's history and sample count and every channel's carry go from block to block.  bins[c] is channel c's
    (signed) bin; several may name the same one."""

    def __init__(self, taps, decim, M, bins, gain=1.0, count=0):
        self.h = np.ascontiguousarray(taps, dtype=np.float32)
        self.R, self.M, self.gain, self.count = int(decim), int(M), float(gain), int(count)
        self.bins = [int(b) for b in bins]
        assert all(-(self.M // 2) <= b <= (self.M - 1) // 2 for b in self.bins)
        self.tw = m17hip.wide_raster_twiddles(self.M)
        self.hist = np.zeros((max(self.h.size - 1, 1), 2), dtype=np.float32)
        self.carry = np.zeros((max(len(self.bins), 1), 2), dtype=np.float32)

    def block(self, row, want_z=False):
        fmt, W, a = wl.fmt_of(row)
        assert W % self.R == 0
        n, nb = W // self.R, len(self.bins)
        k = np.array([b % self.M for b in self.bins], dtype=np.uint32)
        out = np.zeros((nb, n), dtype=np.float32)
        z = np.zeros((nb, n), dtype=np.complex64) if want_z else None
        ok = lib().ro_chan(_p(a), C.c_int(fmt), C.c_size_t(n), C.c_uint32(self.R), _p(self.h), C.c_uint32(self.h.size), C.c_uint32(self.M), _p(self.tw), _p(k),
                           C.c_uint32(nb), C.c_uint64(self.count), _p(self.hist), _p(self.carry), C.c_float(self.gain), _p(out), None if z is None else _p(z))
        assert ok, "M does not factor"
        self.count += W
        return (out, z) if want_z else out


def chan(row, taps, decim, M, bins, gain=1.0, count=0):
    """The floats [len(bins)][n] of one whole feed in one block."""
    return Raster(taps, decim, M, bins, gain, count).block(row)


class Feeds:
    """The device's bookkeeping on the host form: data[S] whole source rows fed block by block; channel c listens to bin[c] of src[c] — both may be rewritten
    between blocks (a channel's carry goes with the channel; history and count are the source's)."""

    def __init__(self, data, taps, decim, M, src, bins, gain):
        self.data, self.R, self.M, self.gain = data, int(decim), int(M), float(gain)
        self.per_source = [Raster(taps, decim, M, [], gain) for _ in range(len(data))]
        self.src, self.bins = list(src), list(bins)
        self.carry = np.zeros((len(self.src), 2), dtype=np.float32)

    def block(self, a, b):
        out = np.zeros((len(self.src), b - a), dtype=np.float32)
        for s, t in enumerate(self.per_source):
            ch = [c for c in range(len(self.src)) if self.src[c] == s]
            t.bins = [int(self.bins[c]) for c in ch]
            t.carry = np.ascontiguousarray(self.carry[ch]) if ch else np.zeros((1, 2), dtype=np.float32)
            y = t.block(self.data[s][a * self.R: b * self.R])
            if ch:
                out[ch] = y
                self.carry[ch] = t.carry
        return out


def chan_channels(x, source, bins, taps, decim, M, gain=1.0):
    """x[S] source rows, one block of a fresh feed -> floats [C][W / decim] for channels (source[c], bins[c])."""
    return Feeds(x, taps, decim, M, source, bins, gain).block(0, wl.fmt_of(x[0])[1] // int(decim))


def samples_f64(row):
    fmt, W, a = wl.fmt_of(row)
    if fmt == wl.IQ_F32:
        return a.astype(np.complex128)
    return a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64) - ((127.5 + 127.5j) if fmt == wl.IQ_U8 else 0.0)


def chan_f64(row, taps, decim, M, b, gain=1.0, count=0, keep=None, residue=0, tap0=0):
    """The whole operation for bin b stated in float64 as the DIRECT sum, with nothing of detail/core.h and no fold in it:
    z[n] = sum_i taps[i] x[m_n - i] exp(-2 pi j k ((count + m_n - i) mod M) / M), k = b mod M, m_n = n R + R - 1, x = 0 in front of the feed;
    y[n] = gain arg(z[n] conj z[n-1]) with y[0] = 0.  Returns (y, z, scale = sum|taps| max|x|).
    What a test hands in to show that a mistake misses the bound: `keep` (default R - 1), the sample of each group of R that is newest; `residue`, added to
    the sample index the phase is taken from; `tap0`, taps dropped from the front (tap i + tap0 meets sample m_n - i)."""
    x = samples_f64(row)
    R, M, W = int(decim), int(M), x.size
    assert W % R == 0
    k = int(b) % M
    m = np.arange(W, dtype=np.int64)
    turns = ((k * ((m + int(count) % M + int(residue)) % M)) % M).astype(np.float64) / M
    mixed = x * np.exp(-2j * np.pi * turns)
    h = np.asarray(taps, dtype=np.float64).reshape(-1)[int(tap0):]
    z = np.convolve(mixed, h)[:W][(R - 1 if keep is None else int(keep))::R]
    y = np.zeros(z.size, dtype=np.float64)
    y[1:] = gain * np.angle(z[1:] * np.conj(z[:-1]))
    return y, z, float(np.abs(np.asarray(taps, dtype=np.float64)).sum() * np.abs(x).max())


def f64_bound(scale, L, M):
    """|z - z_f64| of float32 arithmetic in the channeliser's order.  With X = max|x|, S = sum|taps|, scale = S X, S_r the sum of |taps| on residue r
    (sum_r S_r = S), J = ceil(L / M) and u = 2^-24 (one rounding relative to what is rounded):
      the fold: w[r] is a chain of at most J fma per component, each rounding u of a partial sum of at most S_r X, so a component is off by at most J u S_r X
      and the complex w[r] by sqrt 2 of that; summed over r (every later step has factors of magnitude 1): sqrt 2 J u S X;
      pass 1: every w[r] meets one twiddle, off by at most 2^-25 per component, sqrt 2 2^-25 as a complex factor: sqrt 2 (u / 2) S X over all r; a step of a
      chain rounds twice per component, each u of a partial sum of at most sum|w| over the chain's M2 terms, sqrt 2 for the two components: over all chains
      that feed one z, 2 sqrt 2 M2 u S X;
      pass 2 likewise over M1 steps on sums a with sum|a| <= sum|w| <= S X: sqrt 2 (u / 2) S X + 2 sqrt 2 M1 u S X.
    Together sqrt 2 u scale (J + 2 M1 + 2 M2 + 1); + 1 more for the terms of second order (each below 2^-18 of the first-order ones at these lengths)."""
    m1, m2 = factor_stated(M)
    J = -(-L // M)
    return scale * np.sqrt(2.0) * 2.0 ** -24 * (J + 2 * m1 + 2 * m2 + 2)
