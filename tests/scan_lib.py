"""The HOST form of the carrier scan of m17hip_wide_scan (ABI 622): tests/cxx/scan_oracle.cpp — detail/core.h's scan_peak, scan_distance, scan_fcw,
scan_assign, scan_idle and scan_source under the host compiler — over spectrum_lib's planes and squelch_floor_lib's floor planes, handing squelch_lib's host
form and the tuners' the table they otherwise get from wide_channels.  Beside it the same STATED independently in plain numpy: loops over bins, np.float32
arithmetic step by step, a sort where the definition counts.

TEST INFRASTRUCTURE ONLY, like squelch_floor_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import spectrum_lib as spl
import squelch_floor_lib as sf
import squelch_lib as sql
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "scan_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libscanoracle.so")
SLOT, ASSIGNED, HELD = 1, 2, 4
OPEN = sql.OPEN
_lib = None
_p = wl._p
F = np.float32


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(iq.CORE)):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        for name in ("sc_flag_bits", "sc_max_slots", "sc_distance"):
            getattr(_lib, name).restype = C.c_uint32
        for name in ("sc_peak", "sc_idle", "sc_fcw", "sc_assign"):
            getattr(_lib, name).restype = C.c_int32
        _lib.sc_bands.restype = _lib.sc_block.restype = None
        assert _lib.sc_flag_bits() == SLOT | ASSIGNED << 8 | HELD << 16
    return _lib


def _logn(N):
    logn = int(N).bit_length() - 1
    assert N == 1 << logn
    return logn


# ---- the host form ----------------------------------------------------------------------------------------------------------------------------------------
def bands(row, B):
    """core::squelch_band of every bin of float32 row[N]."""
    row = np.ascontiguousarray(row, dtype=F)
    out = np.zeros(row.size, dtype=F)
    lib().sc_bands(_p(row), C.c_uint32(row.size), C.c_uint32(B), _p(out))
    return out


def peak(band, k, X, to):
    """core::scan_peak."""
    band = np.ascontiguousarray(band, dtype=F)
    return bool(lib().sc_peak(_p(band), C.c_uint32(band.size), C.c_uint32(k), C.c_uint32(X), C.c_float(to)))


def peaks(band, X, to):
    return [k for k in range(len(band)) if peak(band, k, X, to)]


def fcw(row, k, B, med):
    """core::scan_fcw."""
    row = np.ascontiguousarray(row, dtype=F)
    return int(lib().sc_fcw(_p(row), C.c_uint32(row.size), C.c_uint32(_logn(row.size)), C.c_uint32(k), C.c_uint32(B), C.c_float(med)))


def assign(row, band, k, B, med, to):
    """core::scan_assign: scan_fcw with the open guarantee."""
    row, band = np.ascontiguousarray(row, dtype=F), np.ascontiguousarray(band, dtype=F)
    return int(lib().sc_assign(_p(row), _p(band), C.c_uint32(row.size), C.c_uint32(_logn(row.size)), C.c_uint32(k), C.c_uint32(B), C.c_float(med), C.c_float(to)))


def block(plane, J, floor, B, X, hang, src, words, pool, n, hold):
    """One block's scan (what wide_scan_kernel does): plane float32 [S][N] of J frames, floor float32 [4][S], src / words the table in front of the block,
    pool the slot marks [C], n the block's channels, hold the squelch's counts in front of it -> (words int32 [C], flags uint32 [C], missed uint32 [S])."""
    plane = np.ascontiguousarray(plane, dtype=F)
    floor = np.ascontiguousarray(floor, dtype=F)
    S, N = plane.shape
    src = np.ascontiguousarray(src, dtype=np.uint32)
    words = np.ascontiguousarray(words, dtype=np.int32).copy()
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    hold = np.ascontiguousarray(hold, dtype=np.uint32)
    assert floor.shape == (4, S) and src.size == words.size == pool.size == hold.size and n <= src.size
    flags, missed = np.zeros(src.size, dtype=np.uint32), np.zeros(S, dtype=np.uint32)
    lib().sc_block(_p(plane), C.c_uint32(_logn(N)), C.c_uint32(J), C.c_uint32(S), _p(floor), C.c_uint32(B), C.c_uint32(X), C.c_uint32(hang), _p(src),
                   _p(words), _p(pool), C.c_uint32(src.size), C.c_uint32(n), _p(hold), _p(flags), _p(missed))
    return words, flags, missed


# ---- the same, stated ---------------------------------------------------------------------------------------------------------------------------------------
def bands_stated(row, B):
    """band[k] = the chain from +0 of row[(k + d) % N], d = -B .. B ascending: one np.float32 add a step, all bins at once."""
    row = np.asarray(row, dtype=F)
    acc = np.zeros(row.size, dtype=F)
    with np.errstate(all="ignore"):
        for d in range(-int(B), int(B) + 1):
            acc = (acc + np.roll(row, -d)).astype(F)
    return acc


def distance_stated(a, b, N):
    d = (int(a) - int(b)) % N
    return min(d, N - d)


def peak_stated(band, k, X, to):
    N = len(band)
    b = F(band[k])
    if not (b >= F(to)):
        return False
    for j in range(k - X, k + X + 1):
        j %= N
        if j == k:
            continue
        if band[j] > b or (band[j] == b and j < k):
            return False
    return True


def fcw_stated(row, k, B, med):
    row = np.asarray(row, dtype=F)
    N = row.size
    logn = _logn(N)
    sw, sd = F(0.0), F(0.0)
    with np.errstate(all="ignore"):
        for d in range(-int(B), int(B) + 1):
            v = F(row[(k + d) % N] - F(med))
            w = v if v > 0 else F(0.0)
            sw = F(sw + w)
            sd = F(sd + F(F(d) * w))
        delta = F(sd / sw) if sw > 0 else F(0.0)
        if not np.isfinite(delta):
            delta = F(0.0)
        off = int(np.rint(F(delta * F(2.0 ** (32 - logn)))))
    word = ((k << (32 - logn)) + off) & 0xFFFFFFFF
    return word - (1 << 32) if word >= 1 << 31 else word


def assign_stated(row, band, k, B, med, to):
    logn = _logn(len(row))
    w = fcw_stated(row, k, B, med)
    return (k << (32 - logn)) - ((1 << 32) if k >= len(row) // 2 else 0) if band[sql.bin_stated(w, logn)] < F(to) else w


def source_stated(row, J, B, X, open_level, close_level, med, hang, slots, hold, words):
    """One source of one block: slots ascending, hold / words by channel -> ({channel: word} of the assigned, {channel: flags}, missed)."""
    flags = {c: SLOT for c in slots}
    if J == 0 or not np.isfinite(open_level) or not np.isfinite(med):
        return {}, flags, 0
    N = len(row)
    logn = _logn(N)
    with np.errstate(all="ignore"):
        to, tc = F(F(open_level) * F(J)), F(F(close_level) * F(J))
    band = bands_stated(row, B)
    held = [c for c in slots if sql.step_stated(int(hold[c]), band[sql.bin_stated(int(words[c]), logn)], to, tc, hang, J) & OPEN]
    for c in held:
        flags[c] |= HELD
    pk = [k for k in range(N) if band[k] >= to and peak_stated(band, k, X, to)]
    unc = [k for k in pk if not any(distance_stated(sql.bin_stated(int(words[c]), logn), k, N) <= X for c in held)]
    unc.sort(key=lambda k: (-float(band[k]), k))
    free = [c for c in slots if c not in held]
    new = {}
    for c, k in zip(free, unc):
        new[c] = assign_stated(row, band, k, B, med, to)
        flags[c] |= ASSIGNED
    return new, flags, max(0, len(unc) - len(free))


def block_stated(plane, J, floor, B, X, hang, src, words, pool, n, hold):
    words = np.array(words, dtype=np.int64)
    flags = np.array([SLOT if p else 0 for p in pool], dtype=np.uint32)
    missed = np.zeros(len(plane), dtype=np.uint32)
    for s in range(len(plane)):
        slots = [c for c in range(n) if pool[c] and src[c] == s]
        new, fl, missed[s] = source_stated(plane[s], J, B, X, floor[2][s], floor[3][s], floor[0][s], hang, slots, hold, words)
        for c, w in new.items():
            words[c] = w
        for c, v in fl.items():
            flags[c] = v
    return words.astype(np.int32), flags, missed


# ---- a feed ---------------------------------------------------------------------------------------------------------------------------------------------------
class Scan:
    """The slots' words of a feed: `seed` is the host's table (wide_channels), taken by the slots where the feed starts over (fresh) and by every other
    channel in every block."""

    def __init__(self, pool, guard_bins, seed):
        self.pool = np.ascontiguousarray(np.asarray(pool) != 0, dtype=np.uint8)
        self.X = int(guard_bins)
        self.seed = np.ascontiguousarray(seed, dtype=np.int32).copy()
        self.words = self.seed.copy()
        self.fresh = True

    def reset(self):
        self.fresh = True

    def block(self, plane, J, floor, squelch, n=None, stated=False):
        """-> (words int32 [C], flags uint32 [C], missed uint32 [S]); `squelch` is the feed's squelch_lib.Squelch IN FRONT of the block (src, B, hang, hold)."""
        slot = self.pool != 0
        self.words = np.where(slot & (not self.fresh), self.words, self.seed).astype(np.int32)
        self.fresh = False
        fn = block_stated if stated else block
        w, flags, missed = fn(plane, J, floor, squelch.B, self.X, squelch.hang, squelch.src, self.words, self.pool, squelch.src.size if n is None else n,
                              squelch.hold)
        if not stated:
            self.words = w.copy()
        return w, flags, missed


class Feed(sf.Feed):
    """squelch_floor_lib.Feed with the table of every block made by the scan: set .squelch, .floor and .scan.  block(a, b) -> squelch_lib.Feed.block's tuple,
    the floor plane [4][S], and the scan's (words, flags, missed).  `auto_reset`: the channels a block assigns get a zeroed hold count behind it, as
    m17hip_demod_reset_channels leaves them when the caller lists them in front of the block's run."""

    scan = None
    auto_reset = False

    def reset(self, channels=None):
        super().reset(channels)
        if channels is None and self.scan is not None:
            self.scan.reset()

    def block(self, a, b, channels=None):
        got = [spl.plane(self.data[s][a:b], self.N, self.hop, self.win, self.count) for s in range(len(self.data))]
        plane, J = np.stack([g[0] for g in got]), got[0][1]
        keep = self.floor.carry.copy()
        out = self.floor.block(plane, J)
        self.floor.carry[:] = keep   # (sf.Feed.block below steps it again, from the same carry to the same words)
        self.squelch.open, self.squelch.close = out[2].copy(), out[3].copy()
        words, flags, missed = self.scan.block(plane, J, out, self.squelch, channels)
        self.squelch.fcw[:] = words
        for c, t in enumerate(self.tuners):
            t.fcw = int(words[c])
        res = super().block(a, b, channels) + (words, flags, missed)
        ch = [int(c) for c in np.flatnonzero(flags & ASSIGNED)]
        if self.auto_reset and ch:
            self.reset(ch)   # (their IQ carries and hold counts, as the listed form of the reset leaves them)
        return res
