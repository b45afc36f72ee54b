"""The HOST form of the channel meter of m17hip_wide_meter (ABI 618): tests/cxx/meter_oracle.cpp — detail/core.h's meter_pieces, meter_piece, meter_sq,
meter_sum and chan_power under the host compiler — over the z and the y of the host forms of the four wideband configurations (wide_lib.Tuner,
wide2_lib.Tuner2, raster_lib.Raster, resample_lib.Resampler with want_z=True).  Beside it the same stated in Python integers and sequential np.float32 adds.

TEST INFRASTRUCTURE ONLY, like wide_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "meter_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libmeteroracle.so")
GROUP = 16
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
        _lib.mo_group.restype = C.c_uint32
        assert _lib.mo_group() == GROUP
        _lib.mo_sum.restype = C.c_float
        for name in ("mo_pieces", "mo_piece", "mo_power", "mo_plane"):
            getattr(_lib, name).restype = None
    return _lib


def pieces(N0, T, window):
    """(a0, K) of core::meter_pieces."""
    a0, K = C.c_uint32(0), C.c_uint32(0)
    lib().mo_pieces(C.c_uint64(N0), C.c_uint32(T), C.c_uint32(window), C.byref(a0), C.byref(K))
    return a0.value, K.value


def piece(a0, T, window, k):
    """(lo, m) of core::meter_piece."""
    lo, m = C.c_uint32(0), C.c_uint32(0)
    lib().mo_piece(C.c_uint32(a0), C.c_uint32(T), C.c_uint32(window), C.c_uint32(k), C.byref(lo), C.byref(m))
    return lo.value, m.value


def pieces_stated(N0, T, window):
    """[(lo, m)] per piece by brute force in Python integers: the block's outputs n grouped by (N0 + n) div window.  (N0 + n) div window - N0 div window is
    (a0 + n) div window, so this is the definition with the 64-bit count itself in a0's place."""
    out = {}
    for n in range(int(T)):
        out.setdefault((int(N0) + n) // int(window) - int(N0) // int(window), []).append(n)
    assert sorted(out) == list(range(len(out)))
    return [(v[0], len(v)) for _, v in sorted(out.items())]


def msum(v):
    """core::meter_sum of float32 [n]."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return np.float32(lib().mo_sum(_p(v), C.c_uint32(v.size)))


def sum_stated(v):
    """The two-level sum in sequential np.float32 adds: chains from +0 over 16 values each, then the chain from +0 over those."""
    v = np.asarray(v, dtype=np.float32)
    acc = np.float32(0.0)
    for g in range(0, v.size, GROUP):
        q = np.float32(0.0)
        for x in v[g:g + GROUP]:
            q = np.float32(q + x)
        acc = np.float32(acc + q)
    return acc


def power(z):
    """chan_power of complex64 [n]: float32 [n]."""
    z = np.ascontiguousarray(z, dtype=np.complex64).reshape(-1)
    p = np.zeros(z.size, dtype=np.float32)
    lib().mo_power(_p(z), C.c_size_t(z.size), _p(p))
    return p


def plane(p, y, N0, window, edge=0):
    """One channel's block: float32 p[T] and y[T] that begin at output N0 of the feed -> float32 [3][K].  edge: what the definition is NOT
    (meter_oracle.cpp)."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert p.size == y.size and p.size >= 1
    K = pieces(N0, p.size, window)[1]
    out = np.zeros((3, K), dtype=np.float32)
    lib().mo_plane(_p(p), _p(y), C.c_uint32(p.size), C.c_uint64(N0), C.c_uint32(window), C.c_int(edge), _p(out))
    return out


def plane_stated(p, y, N0, window):
    """The same from pieces_stated and sum_stated; e = y * y in np.float32."""
    p = np.asarray(p, dtype=np.float32)
    y = np.asarray(y, dtype=np.float32)
    e = (y * y).astype(np.float32)
    pc = pieces_stated(N0, p.size, window)
    out = np.zeros((3, len(pc)), dtype=np.float32)
    for k, (lo, m) in enumerate(pc):
        for q, v in enumerate((p, y, e)):
            out[q, k] = sum_stated(v[lo:lo + m])
    return out


def planes(P, Y, a, b, N0, window):
    """float32 P[C][n] and Y[C][n] of whole feeds, the block of outputs a .. b - 1 whose first is output N0 of the feed -> float32 [3][C][K]."""
    return np.stack([plane(P[c, a:b], Y[c, a:b], N0, window) for c in range(P.shape[0])], axis=1)


def sum_bound(v, m):
    """|two-level float32 sum - exact sum| of m values of magnitudes v: a value passes through at most 16 adds of the first level and ceil(m / 16) of the
    second, each rounding a partial sum of at most sum|v| (1 + small) by 2^-24 of itself."""
    depth = min(int(m), GROUP) + -(-int(m) // GROUP)
    return float(np.abs(np.asarray(v, dtype=np.float64)).sum()) * depth * 2.0 ** -24 * (1.0 + depth * 2.0 ** -24)
