"""The HOST form of the raster survey of m17hip_wide_survey (ABI 613): the channeliser's z of ALL M bins from raster_lib.Raster(...).block(row, want_z=True)
as it stands, the survey-time rule from N0 and the stride, and tests/cxx/survey_oracle.cpp (detail/core.h's chan_power and the two-level sum under the host
compiler).  Beside it a float64 statement with nothing of core.h in it — sum_j |z64[t_j]|^2 from raster_lib.chan_f64's z — and the derived bound between the
two.

TEST INFRASTRUCTURE ONLY, like raster_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import raster_lib as rl
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "survey_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libsurveyoracle.so")
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
        _lib.so_group.restype = C.c_uint32
        assert _lib.so_group() == GROUP
    return _lib


def times(N0, T, stride, phase=1):
    """The survey times of a block of T outputs that begins at output N0 of the feed: n with (N0 + n + 1) % stride == 0, ascending.  `phase` is what a test
    hands in to show that a mistake misses the bound (0: output n in place of n + 1)."""
    n = np.arange(int(T), dtype=np.int64)
    return n[(int(N0) + n + int(phase)) % int(stride) == 0].astype(np.uint32)


def all_bins(M):
    """The signed bins in the plane's order: entry k is bin k mod M."""
    return [k if k <= (M - 1) // 2 else k - M for k in range(M)]


def plane_of(z, t, single=False):
    """z complex64 [nb][n], survey times t -> float32 [nb]: the two-level sum of chan_power (single: ONE ascending chain, what the definition is not)."""
    z = np.ascontiguousarray(z, dtype=np.complex64)
    t = np.ascontiguousarray(t, dtype=np.uint32)
    assert t.size == 0 or int(t.max()) < z.shape[1]
    out = np.zeros(z.shape[0], dtype=np.float32)
    lib().so_plane(_p(z), C.c_size_t(z.shape[0]), C.c_size_t(z.shape[1]), _p(t), C.c_size_t(t.size), C.c_int(1 if single else 0), _p(out))
    return out


class Survey:
    """ONE source as a feed: history and sample count go from block to block (raster_lib.Raster's), and with them N0."""

    def __init__(self, taps, decim, M, stride, count=0):
        self.r = rl.Raster(taps, decim, M, all_bins(M), 1.0, count)
        self.R, self.M, self.stride = int(decim), int(M), int(stride)

    def block(self, row, single=False):
        """(plane float32 [M] indexed by bin mod M, J, N0) of the next block of the feed."""
        assert self.r.count % self.R == 0
        N0 = self.r.count // self.R
        _, z = self.r.block(row, want_z=True)
        t = times(N0, z.shape[1], self.stride)
        return plane_of(z, t, single), int(t.size), int(N0)


def planes(data, taps, decim, M, stride, cuts):
    """data[S] whole source rows cut at the output indices `cuts` -> per block (plane float32 [S][M], J, N0)."""
    feeds = [Survey(taps, decim, M, stride) for _ in range(len(data))]
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = [f.block(data[s][a * int(decim): b * int(decim)]) for s, f in enumerate(feeds)]
        out.append((np.stack([g[0] for g in got]), got[0][1], got[0][2]))
    return out


def tile_and_lds(L, R, M, stride):
    """csrc/m17_chan_survey_kernels.hpp's survey_wpitch, survey_tile and survey_lds_bytes restated: (survey times per sub-tile, LDS bytes of a workgroup).
    In float2: (TS - 1) WP + L samples with WP = min(stride R, L), M twiddles and two planes of TS rows of M | 1; TS the largest within 32 KB, 16 at the
    most and 1 at the least."""
    wp, mp = min(stride * R, L), M | 1
    size = lambda ts: 8 * ((ts - 1) * wp + L + M + 2 * ts * mp)
    ts = 1
    while ts < GROUP and size(ts + 1) <= 32768:
        ts += 1
    return ts, size(ts)


def depth(J):
    """Float adds a power passes through at the most on its way into P: those of its group's chain and those of the chain of groups."""
    return min(int(J), GROUP) + -(-int(J) // GROUP)


def plane_f64(row, taps, decim, M, stride, count=0, phase=1):
    """One whole feed in one block, in float64 with nothing of detail/core.h in it: P64[k] = sum_j |z64_k[t_j]|^2 from raster_lib.chan_f64's z, and the bound
    on |P_host[k] - P64[k]|, derived as raster_lib.f64_bound is and from the reference alone.  With e = f64_bound (so |z - z64| <= e per survey time),
    a_j = |z64[t_j]|, u = 2^-24 and D = depth(J):
      the error of |z|^2 from the error of z: ||z|^2 - |z64|^2| = |(|z| - |z64|)(|z| + |z64|)| <= e (2 a_j + e);
      the rounding of chan_power = fmaf(re, re, fl(im im)): the product is off by at most u im^2, the fma rounds once more, at most u (|z|^2 + u im^2):
      together at most 2 u (1 + u) |z|^2 <= 2 u (1 + u) (a_j + e)^2;
      the adds: a power passes through at most D of them (min(J, 16) in its group's chain, ceil(J / 16) in the chain of groups — the first of each chain adds
      to +0 and is exact, which the count leaves in), each rounding at most u of a partial sum that is at most the sum of all the (rounded) powers:
      D u (1 + D u) sum_j p_j with p_j <= (1 + 3 u) (a_j + e)^2.
    Returns (P64 float64 [M], bound float64 [M], J)."""
    assert int(count) % int(decim) == 0
    W = wl.fmt_of(row)[1]
    t = times(int(count) // int(decim), W // int(decim), stride, phase)
    u = 2.0 ** -24
    D = depth(t.size)
    L = np.asarray(taps).size
    P, B = np.zeros(M), np.zeros(M)
    for k, b in enumerate(all_bins(M)):
        _, z64, scale = rl.chan_f64(row, taps, decim, M, b, 1.0, count=count)
        e = rl.f64_bound(scale, L, M)
        a = np.abs(z64[t])
        P[k] = float((a * a).sum())
        B[k] = float((e * (2.0 * a + e)).sum() + (2.0 * u * (1.0 + u) + D * u * (1.0 + D * u) * (1.0 + 3.0 * u)) * ((a + e) ** 2).sum())
    return P, B, int(t.size)
