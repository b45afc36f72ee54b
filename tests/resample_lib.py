"""The HOST form of the resampling tuner of m17hip_wide_resample (tests/cxx/resample_oracle.cpp: detail/core.h's ddc_resample under the host compiler), its
float64 statement and the kernel's tile rule restated.  wide_lib and wide2_lib are imported as they stand: their signals and float64 rules are used here.

TEST INFRASTRUCTURE ONLY, like wide2_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "resample_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libresampleoracle.so")
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
        _lib.ro_resample.restype = None
    return _lib


def hist_len(L1, R1, L2, U):
    """Converted samples a source carries from block to block."""
    return (-(-L2 // U) - 1) * R1 + L1 - 1


def row_len(n, R1, U, D):
    """Wideband samples under n outputs (n a multiple of U)."""
    assert n % U == 0
    return n // U * D * R1


PER_LANE, WAVE, LDS_LIMIT = 4, 64, 65536


def tile(L1, R1, L2, U, D):
    """(G, Q, LDS bytes of a workgroup) of resample_kernel, RESTATED from the rule csrc/m17_resample_kernels.hpp describes (not read from it: a change to
    the rule shows as a difference).  A tile is G groups of U outputs.  In complex samples of 8 bytes: one of padding, D planes of G + JD u
    (JD = ceil(ceil(L2 / U) / D)), G U + 1 z and one chunk of R1 planes of 4 Q + J1 - 1 mixed samples (J1 = ceil(L1 / R1)); Q(G) is the most that fits
    64 KB, 64 at the most; G is the value in 1..255 with Q(G) >= 1 that makes (G + JD) / (G Q(G)) smallest, the smallest of equal ones."""
    j1, jd = -(-L1 // R1), -(-(-(-L2 // U)) // D)

    def q_of(G):
        fixed = 1 + D * (G + jd) + G * U + 1
        if fixed >= LDS_LIMIT // 8:
            return 0
        places = (LDS_LIMIT // 8 - fixed) // R1
        return max(min((places + 1 - j1) // PER_LANE, WAVE), 0)

    best, bq = 1, q_of(1)
    assert bq >= 1
    for G in range(2, 256):
        q = q_of(G)
        if q < 1:
            break
        if (G + jd) * best * bq < (best + jd) * G * q:
            best, bq = G, q
    return best, bq, 8 * (1 + D * (best + jd) + best * U + 1 + R1 * (PER_LANE * bq + j1 - 1))


def tile_outputs(L1, R1, L2, U, D):
    """Outputs per tile."""
    return tile(L1, R1, L2, U, D)[0] * U


class Resampler:
    """One channel on one source, as a feed: the source's history, the sample count and the channel's carry go from block to block."""

    def __init__(self, taps1, decim1, up, down, taps2, fcw, gain=1.0, count=0):
        self.h1 = np.ascontiguousarray(taps1, dtype=np.float32)
        self.h2 = np.ascontiguousarray(taps2, dtype=np.float32)
        self.R1, self.U, self.D, self.fcw, self.gain, self.count = int(decim1), int(up), int(down), int(fcw), float(gain), int(count)
        self.hist = np.zeros((max(hist_len(self.h1.size, self.R1, self.h2.size, self.U), 1), 2), dtype=np.float32)
        self.carry = np.zeros(2, dtype=np.float32)

    def outputs(self, W):
        assert W % (self.D * self.R1) == 0
        return W // (self.D * self.R1) * self.U

    def block(self, row, want_z=False):
        fmt, W, a = wl.fmt_of(row)
        n = self.outputs(W)
        out = np.zeros(n, dtype=np.float32)
        z = np.zeros(n, dtype=np.complex64) if want_z else None
        lib().ro_resample(_p(a), C.c_int(fmt), C.c_size_t(n), C.c_uint32(self.R1), _p(self.h1), C.c_uint32(self.h1.size), C.c_uint32(self.U),
                          C.c_uint32(self.D), _p(self.h2), C.c_uint32(self.h2.size), C.c_int32(self.fcw), C.c_uint64(self.count), _p(self.hist),
                          _p(self.carry), C.c_float(self.gain), _p(out), None if z is None else _p(z))
        self.count += W
        return (out, z) if want_z else out


def resample(row, taps1, decim1, up, down, taps2, fcw, gain=1.0):
    """The floats of one whole feed in one block."""
    return Resampler(taps1, decim1, up, down, taps2, fcw, gain).block(row)


class Feeds:
    """wide2_lib.Feeds2 for the resampler: one host-form tuner per channel, fed block by block over data[S] (whole source rows); a and b count OUTPUTS and
    are multiples of `up`; retuning is writing src[c] / fcw[c] (a channel's carry goes with it, the history and the count are the source's)."""

    def __init__(self, data, taps1, decim1, up, down, taps2, src, fcw, gain):
        self.data, self.cfg, self.gain = data, (taps1, int(decim1), int(up), int(down), taps2), float(gain)
        self.R1, self.U, self.D = int(decim1), int(up), int(down)
        self.per_source = [Resampler(*self.cfg, 0, gain) for _ in range(len(data))]   # (for the histories and the count alone)
        self.src, self.fcw = list(src), list(fcw)
        self.carry = [np.zeros(2, dtype=np.float32) for _ in src]

    def block(self, a, b):
        lo, hi = row_len(a, self.R1, self.U, self.D), row_len(b, self.R1, self.U, self.D)
        out = []
        for c in range(len(self.src)):
            s = self.src[c]
            t = Resampler(*self.cfg, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            out.append(t.block(self.data[s][lo:hi]))
            self.carry[c] = t.carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][lo:hi])
        return np.stack(out)


def resample_channels(x, source, fcw, taps1, decim1, up, down, taps2, gain=1.0):
    """x[S] source rows, one block of a fresh feed -> floats [C][outputs] for channels (source[c], fcw[c])."""
    return np.stack([resample(x[s], taps1, decim1, up, down, taps2, w, gain) for s, w in zip(source, fcw)])


def resample_f64(row, taps1, decim1, up, down, taps2, fcw, gain=1.0, phase=0, keep=None):
    """The whole operation stated in float64, with nothing of detail/core.h in it: mixed[m] = x[m] exp(-2 pi j ((fcw m) mod 2^32) / 2^32),
    u = every R1-th of mixed * taps1 (the last of each group), v = u zero-stuffed by U (u[p] at v[U p]), w = v * taps2, z[n] = w[n D + D - 1], all from a
    zero history, y[n] = gain arg(z[n] conj z[n-1]) with y[0] = 0.  Returns (y, z, scale = max_r sum|taps2[r::U]| sum|taps1| max|x|: what one unit of
    relative error in a product is worth in z).  `phase` takes w[n D + D - 1 + phase] (the u of output n then meet the taps i0 + phase + U j) and `keep`
    (default D - 1) is the sample of each group of D that is kept: a test hands in wrong ones to show that they miss the bound."""
    fmt, W, a = wl.fmt_of(row)
    R1, U, D = int(decim1), int(up), int(down)
    assert W % (R1 * D) == 0
    if fmt == wl.IQ_F32:
        x = a.astype(np.complex128)
    else:
        x = a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64) - ((127.5 + 127.5j) if fmt == wl.IQ_U8 else 0.0)
    m = np.arange(W, dtype=np.uint64)
    p = (m * np.uint64(int(fcw) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)   # (m < 2^32: the product fits 64 bits)
    mixed = x * np.exp(-2j * np.pi * (p.astype(np.float64) / 4294967296.0))
    h1 = np.asarray(taps1, dtype=np.float64).reshape(-1)
    h2 = np.asarray(taps2, dtype=np.float64).reshape(-1)
    u = np.convolve(mixed, h1)[:W][R1 - 1::R1]
    v = np.zeros(u.size * U, dtype=np.complex128)
    v[::U] = u
    n = u.size * U // D
    z = np.convolve(v, h2)[(D - 1 if keep is None else int(keep)) + int(phase)::D][:n]
    y = np.zeros(z.size, dtype=np.float64)
    y[1:] = gain * np.angle(z[1:] * np.conj(z[:-1]))
    scale = max(float(np.abs(h2[r::U]).sum()) for r in range(U)) * float(np.abs(h1).sum()) * float(np.abs(x).max())
    return y, z, scale


def f64_bound(scale, L1, L2, U):
    """wide2_lib.f64_bound2 with the taps a z actually meets: ceil(L2 / U) of them, and `scale` made with the largest branch sum."""
    return scale * (2.0 ** -20.5 + (L1 + -(-L2 // U) + 2) * 2.0 ** -24)
