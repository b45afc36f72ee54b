"""The HOST form of the spectrum squelch of m17hip_wide_squelch (ABI 619): tests/cxx/squelch_oracle.cpp — detail/core.h's squelch_bin, squelch_band,
squelch_level and squelch_step under the host compiler — over the spectrum planes of spectrum_lib and the host forms of the three tuners (wide_lib.Tuner,
wide2_lib.Tuner2, resample_lib.Resampler).  Beside it the same stated in Python integers and sequential np.float32 adds.

TEST INFRASTRUCTURE ONLY, like meter_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import meter_lib as ml
import spectrum_lib as spl
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "squelch_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libsquelchoracle.so")
OPEN = 0x80000000
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
        for name in ("so_open_bit", "so_bin", "so_step"):
            getattr(_lib, name).restype = C.c_uint32
        for name in ("so_band", "so_level"):
            getattr(_lib, name).restype = C.c_float
        _lib.so_block.restype = None
        assert _lib.so_open_bit() == OPEN
    return _lib


def bin_(fcw, logn):
    """core::squelch_bin."""
    return int(lib().so_bin(C.c_int32(fcw), C.c_uint32(logn)))


def bin_stated(fcw, logn):
    """The same in Python integers: floor((fcw + 2^(31 - logn)) / 2^(32 - logn)) mod N."""
    return ((int(fcw) + (1 << (31 - logn))) // (1 << (32 - logn))) % (1 << logn)


def band(row, k, B):
    """core::squelch_band of float32 row[N]."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    return np.float32(lib().so_band(_p(row), C.c_uint32(row.size), C.c_uint32(k), C.c_uint32(B)))


def band_stated(row, k, B):
    """The same in sequential np.float32 adds from +0 over d = -B .. B."""
    row = np.asarray(row, dtype=np.float32)
    acc = np.float32(0.0)
    with np.errstate(all="ignore"):
        for d in range(-int(B), int(B) + 1):
            acc = np.float32(acc + row[(int(k) + d) % row.size])
    return acc


def level(lv, J):
    """core::squelch_level."""
    return np.float32(lib().so_level(C.c_float(lv), C.c_uint32(J)))


def step(h, b, to, tc, hang, J):
    """core::squelch_step: h' | open << 31."""
    return int(lib().so_step(C.c_uint32(h), C.c_float(b), C.c_float(to), C.c_float(tc), C.c_uint32(hang), C.c_uint32(J)))


def step_stated(h, b, to, tc, hang, J):
    """The same as the header states it."""
    b, to, tc = np.float32(b), np.float32(to), np.float32(tc)
    if J == 0:
        return h | OPEN
    if not (b < to):
        hn = hang + 1
    elif h > 0 and not (b < tc):
        hn = hang + 1
    else:
        hn = h - 1 if h > 0 else 0
    return hn | (OPEN if hn > 0 else 0)


class Squelch:
    """The decisions of a feed: the hold counts go from block to block."""

    def __init__(self, source, fcw, open_level, close_level, half_bins, hang):
        self.src = np.ascontiguousarray(source, dtype=np.uint32)
        self.fcw = np.ascontiguousarray(fcw, dtype=np.int32)
        self.open = np.ascontiguousarray(open_level, dtype=np.float32)
        self.close = np.ascontiguousarray(close_level, dtype=np.float32)
        self.B, self.hang = int(half_bins), int(hang)
        self.hold = np.zeros(self.src.size, dtype=np.uint32)

    def reset(self, channels=None):
        if channels is None:
            self.hold[:] = 0
        else:
            self.hold[list(channels)] = 0

    def block(self, plane, J, channels=None):
        """plane float32 [S][N] of J frames -> (state uint32 [C], band float32 [C]) of the first `channels` channels; steps their hold counts."""
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        n = self.src.size if channels is None else int(channels)
        logn = int(plane.shape[1]).bit_length() - 1
        assert plane.shape[1] == 1 << logn and self.B < plane.shape[1] // 2
        state, bd = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float32)
        hold = np.ascontiguousarray(self.hold[:n])
        lib().so_block(_p(plane), C.c_uint32(logn), C.c_uint32(J), _p(self.src), _p(self.fcw), C.c_uint32(n), _p(self.open), _p(self.close), C.c_uint32(self.B),
                       C.c_uint32(self.hang), _p(hold), _p(state), _p(bd))
        self.hold[:n] = hold
        return state, bd


class Feed:
    """The squelched host form of a feed of one of the three tuners: tuners[c] is channel c's host form (a Tuner, Tuner2 or Resampler on its source's rows),
    data[S] the whole source rows, N / hop / win the spectrum.  block(a, b) takes the source samples a .. b - 1: the block's spectrum plane, the decision
    (when a Squelch is set), every channel's unsquelched block from its current carry — the histories and counts go on whatever the decision — and, for a
    closed channel, +0 for y and p and a zero carry."""

    def __init__(self, tuners, source, data, N, hop, win=None):
        self.tuners, self.src, self.data, self.N, self.hop, self.win = list(tuners), list(source), data, int(N), int(hop), win
        self.squelch = None
        self.count = 0

    def reset(self, channels=None):
        for c, t in enumerate(self.tuners):
            if channels is None or c in channels:
                t.carry[:] = 0
        if channels is None:
            for t in self.tuners:
                t.hist[:] = 0
                t.count = 0
            self.count = 0
        if self.squelch is not None:
            self.squelch.reset(channels)

    def block(self, a, b, channels=None):
        """-> (Y float32 [C][n], P float32 [C][n], state uint32 [C] or None, band float32 [C] or None, J)."""
        n = len(self.tuners) if channels is None else int(channels)
        got = [spl.plane(self.data[s][a:b], self.N, self.hop, self.win, self.count) for s in range(len(self.data))]
        plane, J = np.stack([g[0] for g in got]), got[0][1]
        state = bd = None
        if self.squelch is not None:
            state, bd = self.squelch.block(plane, J, n)
        Y, P = [], []
        for c in range(len(self.tuners)):   # (the channels beyond the launch's keep their carry; their source's history goes on)
            t = self.tuners[c]
            if c >= n:
                keep = t.carry.copy()
                t.block(self.data[self.src[c]][a:b])
                t.carry[:] = keep
                continue
            y, z = t.block(self.data[self.src[c]][a:b], want_z=True)
            p = ml.power(z)
            if state is not None and not (int(state[c]) & OPEN):
                y, p = np.zeros_like(y), np.zeros_like(p)
                t.carry[:] = 0
            Y.append(y)
            P.append(p)
        self.count += b - a
        return np.stack(Y), np.stack(P), state, bd, J
