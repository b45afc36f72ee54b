"""The HOST form of the two-stage tuner of m17hip_wide_config2 (tests/cxx/wide2_oracle.cpp: detail/core.h's ddc_mix / ddc_fir2 under the host compiler, the
discriminator behind them), its float64 statement and the checks of the default first-stage taps.  wide_lib is imported as it stands: its signals, its
single-stage Tuner and its float64 rules are used here.

TEST INFRASTRUCTURE ONLY, like wide_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "wide2_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libwide2oracle.so")
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
        _lib.wo2_tune.restype = None
    return _lib


def hist_len(L1, R1, L2):
    """Converted samples a source carries from block to block."""
    return (L2 - 1) * R1 + L1 - 1


TILE_Z, PER_LANE, WAVE, LDS_LIMIT = 256, 4, 64, 65536


def q_and_lds(L1, R1, L2, R2):
    """(Q, LDS bytes of a workgroup) of tune2_kernel, RESTATED from the layout csrc/m17_wide2_kernels.hpp describes (not read from it: a change to
    wide2_q shows as a difference).  In complex samples of 8 bytes: R2 planes of 255 + J2 u, the tile's 256 z and one chunk of R1 planes of 4 Q + J1 - 1
    mixed samples, J = ceil(L / R); Q is the most that fits 64 KB, and 64 at the most."""
    j1, j2 = -(-L1 // R1), -(-L2 // R2)
    fixed = R2 * (TILE_Z - 1 + j2) + TILE_Z
    places = (LDS_LIMIT // 8 - fixed) // R1
    q = min((places + 1 - j1) // PER_LANE, WAVE)
    return q, 8 * (fixed + R1 * (PER_LANE * q + j1 - 1))


class Tuner2:
    """One channel on one source in two stages, as a feed: the source's history, the sample count and the channel's carry go from block to block."""

    def __init__(self, taps1, decim1, taps2, decim2, fcw, gain=1.0, count=0):
        self.h1 = np.ascontiguousarray(taps1, dtype=np.float32)
        self.h2 = np.ascontiguousarray(taps2, dtype=np.float32)
        self.R1, self.R2, self.fcw, self.gain, self.count = int(decim1), int(decim2), int(fcw), float(gain), int(count)
        self.R = self.R1 * self.R2
        self.hist = np.zeros((max(hist_len(self.h1.size, self.R1, self.h2.size), 1), 2), dtype=np.float32)
        self.carry = np.zeros(2, dtype=np.float32)

    def block(self, row, want_z=False):
        fmt, W, a = wl.fmt_of(row)
        assert W % self.R == 0
        n = W // self.R
        out = np.zeros(n, dtype=np.float32)
        z = np.zeros(n, dtype=np.complex64) if want_z else None
        lib().wo2_tune(_p(a), C.c_int(fmt), C.c_size_t(n), C.c_uint32(self.R1), _p(self.h1), C.c_uint32(self.h1.size), C.c_uint32(self.R2), _p(self.h2),
                       C.c_uint32(self.h2.size), C.c_int32(self.fcw), C.c_uint64(self.count), _p(self.hist), _p(self.carry), C.c_float(self.gain), _p(out),
                       None if z is None else _p(z))
        self.count += W
        return (out, z) if want_z else out


def tune2(row, taps1, decim1, taps2, decim2, fcw, gain=1.0):
    """The floats of one whole feed in one block."""
    return Tuner2(taps1, decim1, taps2, decim2, fcw, gain).block(row)


class Feeds2:
    """wide_lib.Feeds in two stages: one host-form tuner per channel, fed block by block over data[S] (whole source rows); retuning is writing src[c] /
    fcw[c] (a channel's carry goes with it, the history and the count are the source's)."""

    def __init__(self, data, taps1, decim1, taps2, decim2, src, fcw, gain):
        self.data, self.cfg, self.gain = data, (taps1, int(decim1), taps2, int(decim2)), float(gain)
        self.R = int(decim1) * int(decim2)
        self.per_source = [Tuner2(*self.cfg, 0, gain) for _ in range(len(data))]   # (for the histories and the count alone)
        self.src, self.fcw = list(src), list(fcw)
        self.carry = [np.zeros(2, dtype=np.float32) for _ in src]

    def block(self, a, b):
        out = []
        for c in range(len(self.src)):
            s = self.src[c]
            t = Tuner2(*self.cfg, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            out.append(t.block(self.data[s][a * self.R: b * self.R]))
            self.carry[c] = t.carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][a * self.R: b * self.R])
        return np.stack(out)


def tune2_channels(x, source, fcw, taps1, decim1, taps2, decim2, gain=1.0):
    """x[S] source rows, one block of a fresh feed -> floats [C][W / (decim1 decim2)] for channels (source[c], fcw[c])."""
    return np.stack([tune2(x[s], taps1, decim1, taps2, decim2, w, gain) for s, w in zip(source, fcw)])


def tune2_f64(row, taps1, decim1, taps2, decim2, fcw, gain=1.0, keep1=None, keep2=None):
    """The whole two-stage operation stated in float64, with nothing of detail/core.h in it: mixed[m] = x[m] exp(-2 pi j ((fcw m) mod 2^32) / 2^32),
    u[p] = sum_i taps1[i] mixed[p R1 + R1 - 1 - i] and z[n] = sum_i taps2[i] u[n R2 + R2 - 1 - i], both from a zero history, y[n] = gain arg(z[n] conj
    z[n-1]) with y[0] = 0.  Returns (y, z, scale = sum|taps2| sum|taps1| max|x|: what one unit of relative error in a product is worth in z).  `keep1` /
    `keep2` (default R1 - 1 / R2 - 1) is the sample of each group that a stage keeps: a test hands in another one to show that a wrong decimation phase
    in either stage misses the bound."""
    fmt, W, a = wl.fmt_of(row)
    R1, R2 = int(decim1), int(decim2)
    assert W % (R1 * R2) == 0
    if fmt == wl.IQ_F32:
        x = a.astype(np.complex128)
    else:
        x = a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64) - ((127.5 + 127.5j) if fmt == wl.IQ_U8 else 0.0)
    m = np.arange(W, dtype=np.uint64)
    p = (m * np.uint64(int(fcw) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)   # (m < 2^32: the product fits 64 bits)
    mixed = x * np.exp(-2j * np.pi * (p.astype(np.float64) / 4294967296.0))
    h1 = np.asarray(taps1, dtype=np.float64).reshape(-1)
    h2 = np.asarray(taps2, dtype=np.float64).reshape(-1)
    u = np.convolve(mixed, h1)[:W][(R1 - 1 if keep1 is None else int(keep1))::R1]
    z = np.convolve(u, h2)[:u.size][(R2 - 1 if keep2 is None else int(keep2))::R2]
    y = np.zeros(z.size, dtype=np.float64)
    y[1:] = gain * np.angle(z[1:] * np.conj(z[:-1]))
    return y, z, float(np.abs(h2).sum() * np.abs(h1).sum() * np.abs(x).max())


def f64_bound2(scale, L1, L2):
    """|z - z_f64| of float32 arithmetic in the two-stage tuner's order, derived as wide_lib.f64_bound is.  With X = max|x|, S1 = sum|taps1|, S2 = sum|taps2|
    and scale = S2 S1 X:
      a mixed sample is off by at most X (2^-20.5 + 2 2^-24): the oscillator's asserted 2^-21 on both components (sqrt 2 of it on the complex factor) and two
      roundings for the cross product;
      a u is a sum of L1 of them weighted by taps1, so it inherits S1 times that, and its fma chain rounds once per tap, each rounding 2^-24 of a partial sum
      of at most S1 X: |u - u_f64| <= S1 X (2^-20.5 + (L1 + 2) 2^-24);
      a z is a sum of L2 u weighted by taps2: S2 times the u's error, plus one rounding per tap of 2^-24 of a partial sum of at most S2 S1 X.
    Together scale (2^-20.5 + (L1 + L2 + 2) 2^-24)."""
    return scale * (2.0 ** -20.5 + (L1 + L2 + 2) * 2.0 ** -24)


def f64_ok(z64, bound):
    """Outputs the y rule of wide_lib.f64_check_y speaks about: z[n] and z[n-1] of the reference both above 8 bound."""
    mag = np.abs(z64)
    ok = np.zeros(mag.size, dtype=bool)
    ok[1:] = (mag[1:] > 8.0 * bound) & (mag[:-1] > 8.0 * bound)
    return ok


def f64_errors(y, z, y64, z64, bound, gain):
    """(the largest |z - z_f64| over its bound, the largest |y - y_f64| mod 2 pi gain over ITS bound gain (2 bound / min|z| + 2^-20) — wide_lib.f64_check_y's
    rule —, the share of outputs that rule does not speak about)."""
    ok = f64_ok(z64, bound)
    mag = np.abs(z64)
    ez = float(np.abs(np.asarray(z).astype(np.complex128) - z64).max()) / bound
    lowest = np.minimum(mag[1:], mag[:-1])[ok[1:]]
    dy = np.abs(np.angle(np.exp(1j * (np.asarray(y, dtype=np.float64) - y64) / gain)))[ok] * gain
    ey = float((dy / (gain * (2.0 * bound / lowest + 2.0 ** -20))).max())
    return ez, ey, 1.0 - float(ok.mean())


def response_db(taps, rate_hz, hz):
    """20 log10 |H| of the taps at the frequencies `hz` (array) for a sample rate of rate_hz, in float64."""
    h = np.asarray(taps, dtype=np.float64)
    w = np.exp(-2j * np.pi * np.outer(np.asarray(hz, dtype=np.float64) / rate_hz, np.arange(h.size)))
    return 20.0 * np.log10(np.maximum(np.abs(w @ h), 1e-300))
