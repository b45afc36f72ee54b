"""The HOST form of the source spectrum of m17hip_wide_spectrum (ABI 616): tests/cxx/spectrum_oracle.cpp — detail/core.h's spec_frames, spec_window,
spec_bitrev, spec_item1 / spec_item2, chan_power and the two-level sum under the host compiler — over a source row converted as the device converts it.
Beside it a float64 statement with nothing of core.h in it — np.fft.fft of the window times the samples, |.|^2 summed over frames found by Python
integers — and the derived bound between the two.

TEST INFRASTRUCTURE ONLY, like survey_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import survey_lib as sl
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "spectrum_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libspectrumoracle.so")
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
        _lib.sp_group.restype = C.c_uint32
        assert _lib.sp_group() == GROUP
        for name in ("sp_frames", "sp_fft", "sp_plane"):
            getattr(_lib, name).restype = None
    return _lib


def floats(row):
    """One source row as the device's floats, float32 [W][2]: int16 and float32 as they are, uint8 minus 127.5 (all exact)."""
    fmt, W, a = wl.fmt_of(row)
    if fmt == wl.IQ_F32:
        return np.ascontiguousarray(a.view(np.float32).reshape(W, 2))
    if fmt == wl.IQ_I16:
        return np.ascontiguousarray(a.astype(np.float32))
    return np.ascontiguousarray(a.astype(np.float32) - np.float32(127.5))


def frames(c0, W, N, hop):
    """(first, J) of core::spec_frames."""
    first, J = C.c_uint32(0), C.c_uint32(0)
    lib().sp_frames(C.c_uint64(c0), C.c_uint32(W), C.c_uint32(N), C.c_uint32(hop), C.byref(first), C.byref(J))
    return first.value, J.value


def frames_stated(c0, W, N, hop):
    """The same by brute force in Python integers: the block samples a whose feed index c0 + a is a multiple of hop and whose frame ends inside the block."""
    starts = [a for a in range(max(int(W) - int(N) + 1, 0)) if (int(c0) + a) % int(hop) == 0]
    return (starts[0] if starts else (int(hop) - int(c0) % int(hop)) % int(hop)), len(starts)


def window(N):
    return __import__("m17hip").wide_spectrum_default_window(N)


def twiddles(N):
    return __import__("m17hip").wide_spectrum_twiddles(N)


def fft(v, fused=False):
    """The host form's DFT of complex64 [N] (N a power of two >= 4)."""
    v = np.ascontiguousarray(v, dtype=np.complex64).copy()
    logn = int(v.size).bit_length() - 1
    assert v.size == 1 << logn
    tw = twiddles(v.size) if v.size >= 64 else np.exp(-2j * np.pi * np.arange(v.size // 2) / v.size).astype(np.complex64)
    lib().sp_fft(_p(v), _p(tw), C.c_uint32(logn), C.c_int(1 if fused else 0))
    return v


def plane(row, N, hop, win=None, c0=0, shift=0, wshift=0, single=False, fused=False):
    """(plane float32 [N], J, first) of one block that begins at sample c0 of the feed.  shift, wshift, single: what the definition is NOT
    (spectrum_oracle.cpp)."""
    x = floats(row)
    logn = int(N).bit_length() - 1
    assert N == 1 << logn
    w = np.ascontiguousarray(window(N) if win is None else win, dtype=np.float32)
    assert w.size == N
    tw = twiddles(N)
    out = np.zeros(N, dtype=np.float32)
    first, J = C.c_uint32(0), C.c_uint32(0)
    f0, j0 = frames(c0, x.shape[0], N, hop)
    assert j0 == 0 or (f0 + shift >= 0 and f0 + (j0 - 1) * hop + shift + N <= x.shape[0])
    lib().sp_plane(_p(x), C.c_uint32(x.shape[0]), C.c_uint64(c0), _p(w), _p(tw), C.c_uint32(logn), C.c_uint32(hop), C.c_int(shift), C.c_int(wshift),
                   C.c_int(1 if single else 0), C.c_int(1 if fused else 0), _p(out), C.byref(first), C.byref(J))
    return out, int(J.value), int(first.value)


def planes(data, N, hop, cuts, win=None, c0=0):
    """data[S] whole source rows cut at the sample indices `cuts` -> per block (plane float32 [S][N], J, c0 + first of that block)."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        got = [plane(data[s][a:b], N, hop, win, c0 + a) for s in range(len(data))]
        out.append((np.stack([g[0] for g in got]), got[0][1], c0 + a + got[0][2]))
    return out


def plane_f64(row, N, hop, win, c0=0):
    """One block in float64 with nothing of detail/core.h in it: P64[k] = sum_f |FFT(w x[a_f : a_f + N])[k]|^2 over the frames Python integers find, and the
    bound on |P_host[k] - P64[k]|, derived from the reference alone.  With u = 2^-24, A_f = sum_i |w[i] x[a_f + i]| (the frame's L1 norm), n = log2 N:
      the window: fl(w re), fl(w im) are each off by at most u of themselves, so v is off by at most u |v| and X by at most u A_f;
      a butterfly (a, b) <- (a +- b t): the table's t is the double's rounded, off by at most u per component (the double's own error, 2^-53, is left to
      the slack below), which moves b t by at most u |b|; a component of the result is two fma deep, each rounding at most u of a partial result that is at
      most |a| + |b| (|re b re t| + |im b im t| <= |b| |t| by Cauchy-Schwarz, and likewise for the imaginary chain), so a component is off by at most
      2 u (|a| + |b|) and the complex result by sqrt(2) times that, below 4 u (|a| + |b|); together 5 u (|a| + |b|) per butterfly;
      every element of stage s is a sum of 2^s of the v, each times a number of modulus 1, so |a| + |b| of a butterfly is at most the L1 norm of the v it
      covers; the butterflies of one stage that X[k] depends on cover disjoint v: a stage adds at most 5 u A_f to the error of X[k], the n stages 5 n u A_f;
      e_f = (5 n + 1) u A_f (1 + 2^-10) — the factor covers the second-order terms: the computed magnitudes in place of the exact ones, the errors carried
      through later butterflies' products (each at most (1 + 6 u) per stage), the double's 2^-53;
      the power: ||X|^2 - |X64|^2| <= e_f (2 |X64| + e_f); chan_power's own rounding 2 u (1 + u) (|X64| + e_f)^2; the adds D u (1 + D u) (1 + 3 u) of the
      sum of (|X64| + e_f)^2, D = survey_lib.depth(J) — as survey_lib.plane_f64 derives them.
    Returns (P64 float64 [N], bound float64 [N], J, first)."""
    x = floats(row).astype(np.float64)
    x = x[:, 0] + 1j * x[:, 1]
    w = np.asarray(win, dtype=np.float64)
    first, J = frames_stated(c0, x.size, N, hop)
    u = 2.0 ** -24
    n = int(N).bit_length() - 1
    D = sl.depth(J)
    P, E1, E2 = np.zeros(N), np.zeros(N), np.zeros(N)
    for f in range(J):
        v = w * x[first + f * hop: first + f * hop + N]
        X = np.abs(np.fft.fft(v))
        e = (5 * n + 1) * u * float(np.abs(v).sum()) * (1.0 + 2.0 ** -10)
        P += X * X
        E1 += e * (2.0 * X + e)
        E2 += (X + e) ** 2
    return P, E1 + (2.0 * u * (1.0 + u) + D * u * (1.0 + D * u) * (1.0 + 3.0 * u)) * E2, J, first


def frames_per_pass_and_lds(N):
    """csrc/m17_spectrum_kernels.hpp's spectrum_frames_per_pass and spectrum_lds_bytes restated: (frames a pass holds, LDS bytes of a workgroup)."""
    F = min(max(2048 // N, 1), GROUP)
    return F, 8 * (F * N + N // 2)
