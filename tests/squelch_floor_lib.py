"""The HOST form of the sources' noise floor of m17hip_wide_squelch_floor (ABI 621): tests/cxx/squelch_floor_oracle.cpp — detail/core.h's squelch_floor_key,
squelch_floor_median, squelch_floor, squelch_track and squelch_floor_level under the host compiler — over spectrum_lib's planes, feeding squelch_lib's and
squelch_slots_lib's host forms the levels they otherwise get as given levels.  Beside it the same stated in Python integers and numpy.

TEST INFRASTRUCTURE ONLY, like squelch_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import spectrum_lib as spl
import squelch_lib as sql
import squelch_slots_lib as ssl
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "squelch_floor_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libsquelchfloororacle.so")
NAN = 0x7FC00000
OPEN = sql.OPEN
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
        for name in ("sf_key", "sf_nan"):
            getattr(_lib, name).restype = C.c_uint32
        for name in ("sf_median", "sf_floor", "sf_track", "sf_level"):
            getattr(_lib, name).restype = C.c_float
        _lib.sf_block.restype = None
        assert _lib.sf_nan() == NAN
    return _lib


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(word):
    return np.array([word], dtype=np.uint32).view(np.float32)[0]


def key(x):
    """core::squelch_floor_key."""
    return int(lib().sf_key(C.c_float(x)))


def keys_stated(row):
    """The keys of float32 row[N] as uint32: the word, 0xFFFFFFFF for every NaN."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    return np.where(np.isnan(row), np.uint32(0xFFFFFFFF), row.view(np.uint32)).astype(np.uint32)


def median(row):
    """core::squelch_floor_median of float32 row[N], as a word."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    out = np.zeros((4, 1), dtype=np.float32)
    carry = np.array([np.nan], dtype=np.float32)
    lib().sf_block(_p(row), C.c_uint32(row.size), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0), C.c_float(1.0), C.c_float(1.0), C.c_float(1.0),
                   C.c_float(1.0), C.c_float(0.0), _p(carry), _p(out))
    return int(out.view(np.uint32)[0, 0])


def median_stated(row):
    """The same in Python integers: the key of rank N // 2 of the sorted keys, 0x7FC00000 where it is 0xFFFFFFFF."""
    k = sorted(int(v) for v in keys_stated(row))[len(row) // 2]
    return NAN if k == 0xFFFFFFFF else k


def floor(med, B, J, floor_min):
    """core::squelch_floor."""
    return np.float32(lib().sf_floor(C.c_float(med), C.c_uint32(B), C.c_uint32(J), C.c_float(floor_min)))


def floor_stated(med, B, J, floor_min):
    with np.errstate(all="ignore"):
        f = np.float32(np.float32(np.float32(med) * np.float32(2 * int(B) + 1)) / np.float32(int(J)))
    return np.float32(floor_min) if f < np.float32(floor_min) else f


def track(F, f, rise, fall):
    """core::squelch_track."""
    return np.float32(lib().sf_track(C.c_float(F), C.c_float(f), C.c_float(rise), C.c_float(fall)))


def fma32(a, b, c):
    """fmaf of three float32: the products and sums of float32 are exact in float64 only up to 48 + bits, so in Python's exact rationals, rounded once."""
    from fractions import Fraction
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return _round_f32(v)


def _round_f32(v):
    """A rational rounded to the nearest float32, ties to even (finite results in the normal and subnormal range)."""
    from fractions import Fraction
    if v == 0:
        return np.float32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = 0
    while v >= 2:
        v /= 2
        e += 1
    while v < 1:
        v *= 2
        e -= 1
    e0 = max(e, -126)                         # (subnormals keep the exponent of the smallest normal)
    q = v * Fraction(2) ** (e - e0) * (1 << 23)
    n = int(q)
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(Fraction(n, 1 << 23) * Fraction(2) ** e0))


def track_stated(F, f, rise, fall):
    F, f = np.float32(F), np.float32(f)
    if not (F == F):
        return f
    if not np.isfinite(f):
        return F
    a = np.float32(rise) if f > F else np.float32(fall)
    if a >= np.float32(1.0):
        return f
    with np.errstate(all="ignore"):
        d = np.float32(f - F)
    return fma32(a, d, F)


class Floor:
    """The floors of a feed: the carry goes from block to block, a NaN in front of the first."""

    def __init__(self, sources, half_bins, open_ratio, close_ratio, rise=1.0, fall=1.0, floor_min=0.0):
        self.S, self.B = int(sources), int(half_bins)
        self.open_ratio, self.close_ratio = np.float32(open_ratio), np.float32(close_ratio)
        self.rise, self.fall, self.floor_min = np.float32(rise), np.float32(fall), np.float32(floor_min)
        self.carry = np.full(self.S, f32(NAN), dtype=np.float32)

    def reset(self):
        self.carry[:] = f32(NAN)

    def block(self, plane, J):
        """plane float32 [S][N] of J frames -> out float32 [4][S] = med | F' | open | close; steps the carry."""
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        assert plane.shape[0] == self.S
        out = np.zeros((4, self.S), dtype=np.float32)
        lib().sf_block(_p(plane), C.c_uint32(plane.shape[1]), C.c_uint32(J), C.c_uint32(self.S), C.c_uint32(self.B), C.c_float(self.open_ratio),
                       C.c_float(self.close_ratio), C.c_float(self.rise), C.c_float(self.fall), C.c_float(self.floor_min), _p(self.carry), _p(out))
        return out

    def block_stated(self, plane, J, carry):
        """The same from `carry` (not stepped), stated."""
        out = np.zeros((4, self.S), dtype=np.float32)
        for s in range(self.S):
            med = f32(median_stated(plane[s]))
            F = np.float32(carry[s])
            if J:
                F = track_stated(F, floor_stated(med, self.B, J, self.floor_min), self.rise, self.fall)
            with np.errstate(all="ignore"):
                out[:, s] = [med, F, np.float32(F * self.open_ratio), np.float32(F * self.close_ratio)]
        return out


class Feed(sql.Feed):
    """squelch_lib.Feed with the levels of every block made from the block's own plane: set .squelch (a squelch_lib.Squelch; its levels are overwritten per
    block) and .floor (a Floor).  block(a, b) -> squelch_lib.Feed.block's tuple and the floor plane [4][S]."""

    floor = None

    def reset(self, channels=None):
        super().reset(channels)
        if channels is None and self.floor is not None:
            self.floor.reset()

    def block(self, a, b, channels=None):
        got = [spl.plane(self.data[s][a:b], self.N, self.hop, self.win, self.count) for s in range(len(self.data))]
        plane, J = np.stack([g[0] for g in got]), got[0][1]
        out = self.floor.block(plane, J)
        self.squelch.open, self.squelch.close = out[2].copy(), out[3].copy()
        return super().block(a, b, channels) + (out,)


class SlotFeed(ssl.Feed):
    """squelch_slots_lib.Feed likewise: the floor is taken from the block's plane — the second-level sum, not a slot's row — and serves all its slots."""

    floor = None

    def reset(self, channels=None):
        super().reset(channels)
        if channels is None and self.floor is not None:
            self.floor.reset()

    def block(self, a, b, channels=None):
        got = [spl.plane(self.data[s][a:b], self.N, self.hop, self.win, self.count) for s in range(len(self.data))]
        plane, J = np.stack([g[0] for g in got]), got[0][1]
        out = self.floor.block(plane, J)
        self.squelch.open, self.squelch.close = out[2].copy(), out[3].copy()
        return super().block(a, b, channels) + (out,)
