"""The HOST form of the time-resolved squelch of m17hip_wide_squelch_slots (ABI 620): tests/cxx/squelch_slots_oracle.cpp — detail/core.h's squelch_slots,
squelch_slot_frames, squelch_slot_of, squelch_tile_span and squelch_tile_open under the host compiler — over spectrum_lib's group sums and the host forms of
the three tuners (wide_lib.Tuner, wide2_lib.Tuner2, resample_lib.Resampler).  Beside it the same stated in Python integers and, through squelch_lib's stated
functions, sequential np.float32 adds.

TEST INFRASTRUCTURE ONLY, like squelch_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import iq_lib as iq
import meter_lib as ml
import spectrum_lib as spl
import squelch_lib as sql
import wide_lib as wl

SRC = os.path.join(wl.ROOT, "tests", "cxx", "squelch_slots_oracle.cpp")
LIB = os.path.join(wl.ROOT, "tests", "cxx", "libsquelchslotsoracle.so")
OPEN = sql.OPEN
GROUP = spl.GROUP
WIDE_TILE = 255
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
        for name in ("ss_slots", "ss_slot_frames", "ss_slot_of", "ss_tile_open"):
            getattr(_lib, name).restype = C.c_uint32
        _lib.ss_tile_span.restype = None
        _lib.ss_block.restype = None
    return _lib


def slots(J):
    return int(lib().ss_slots(C.c_uint32(J)))


def slots_stated(J):
    return -(-int(J) // GROUP)


def slot_frames(J, g):
    return int(lib().ss_slot_frames(C.c_uint32(J), C.c_uint32(g)))


def slot_frames_stated(J, g):
    return min(GROUP, int(J) - GROUP * int(g))


def slot_of(x, first, hop, G):
    return int(lib().ss_slot_of(C.c_uint32(x), C.c_uint32(first), C.c_uint32(hop), C.c_uint32(G)))


def slot_of_stated(x, first, hop, G):
    return 0 if x < first else min((int(x) - int(first)) // (GROUP * int(hop)), int(G) - 1)


def tile_span(t, TO, T, W):
    a, e = C.c_uint32(0), C.c_uint32(0)
    lib().ss_tile_span(C.c_uint32(t), C.c_uint32(TO), C.c_uint32(T), C.c_uint32(W), C.byref(a), C.byref(e))
    return a.value, e.value


def tile_span_stated(t, TO, T, W):
    return int(t) * int(TO) * int(W) // int(T), min((int(t) + 1) * int(TO), int(T)) * int(W) // int(T)


def pack(flags):
    """bool [n] -> uint32 words, bit i & 31 of word i >> 5 (one word at least)."""
    flags = np.asarray(flags, dtype=bool)
    out = np.zeros(max((flags.size + 31) // 32, 1), dtype=np.uint32)
    for i in np.flatnonzero(flags):
        out[i >> 5] |= np.uint32(1 << (int(i) & 31))
    return out


def unpack(words, n):
    """uint32 words [..., MW] -> bool [..., n]."""
    words = np.asarray(words, dtype=np.uint32)
    i = np.arange(int(n))
    return ((words[..., i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def tile_open(open_flags, first, hop, lead, a, e):
    G = len(open_flags)
    bits = pack(open_flags)
    return bool(lib().ss_tile_open(_p(bits), C.c_uint32(G), C.c_uint32(first), C.c_uint32(hop), C.c_uint32(lead), C.c_uint32(a), C.c_uint32(e)))


def tile_open_stated(open_flags, first, hop, lead, a, e):
    G = len(open_flags)
    if G == 0:
        return True
    g0, g1 = slot_of_stated(a, first, hop, G), min(slot_of_stated(e - 1, first, hop, G) + int(lead), G - 1)
    return any(bool(open_flags[g]) for g in range(g0, g1 + 1))


def slot_rows(row, N, hop, win=None, c0=0):
    """(rows float32 [G][N], J, first) of one source block that begins at sample c0 of the feed: slot g's row is spectrum_lib's plane of the slot's frames
    alone — a plane of at most 16 frames is its one group's first-level sum (the second level adds it to +0, and no power is -0)."""
    fmt, W, _ = wl.fmt_of(row)
    first, J = spl.frames(c0, W, N, hop)
    G = slots_stated(J)
    out = np.zeros((G, N), dtype=np.float32)
    for g in range(G):
        a, jg = first + GROUP * g * hop, slot_frames_stated(J, g)
        got, j, f = spl.plane(row[a:a + (jg - 1) * hop + N], N, hop, win, 0)
        assert j == jg and f == 0
        out[g] = got
    return out, J, first


class SlotSquelch:
    """The decisions of a feed: the hold counts go from block to block."""

    def __init__(self, source, fcw, open_level, close_level, half_bins, hang, lead):
        self.src = np.ascontiguousarray(source, dtype=np.uint32)
        self.fcw = np.ascontiguousarray(fcw, dtype=np.int32)
        self.open = np.ascontiguousarray(open_level, dtype=np.float32)
        self.close = np.ascontiguousarray(close_level, dtype=np.float32)
        self.B, self.hang, self.lead = int(half_bins), int(hang), int(lead)
        self.hold = np.zeros(self.src.size, dtype=np.uint32)

    def reset(self, channels=None):
        if channels is None:
            self.hold[:] = 0
        else:
            self.hold[list(channels)] = 0

    def block(self, rows, J, first, hop, TO, T, W, channels=None):
        """rows float32 [S][G][N] -> (state uint32 [C], bands float32 [C][G], open bool [C][G], mask uint32 [C][MW], tiles) of the first `channels`
        channels; steps their hold counts."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = self.src.size if channels is None else int(channels)
        G, N = rows.shape[1], rows.shape[2]
        logn = int(N).bit_length() - 1
        assert N == 1 << logn and self.B < N // 2 and G == slots_stated(J)
        tiles = -(-int(T) // int(TO))
        SW, MW = max((G + 31) // 32, 1), (tiles + 31) // 32
        state, bd = np.zeros(n, dtype=np.uint32), np.zeros((n, G), dtype=np.float32)
        bits, mask = np.zeros((n, SW), dtype=np.uint32), np.zeros((n, MW), dtype=np.uint32)
        hold = np.ascontiguousarray(self.hold[:n])
        lib().ss_block(_p(rows), C.c_uint32(logn), C.c_uint32(J), C.c_uint32(first), C.c_uint32(hop), _p(self.src), _p(self.fcw), C.c_uint32(n), _p(self.open),
                       _p(self.close), C.c_uint32(self.B), C.c_uint32(self.hang), C.c_uint32(self.lead), C.c_uint32(TO), C.c_uint32(T), C.c_uint32(W),
                       C.c_uint32(tiles), _p(hold), _p(state), _p(bd), _p(bits), _p(mask))
        self.hold[:n] = hold
        return state, bd, unpack(bits, G), mask, tiles

    def block_stated(self, rows, J, first, hop, TO, T, W, hold):
        """The same from `hold` (not stepped) in Python integers and squelch_lib's stated band and step: (state, bands, open, tile flags bool [C][tiles])."""
        rows = np.asarray(rows, dtype=np.float32)
        G, N = rows.shape[1], rows.shape[2]
        logn = int(N).bit_length() - 1
        tiles = -(-int(T) // int(TO))
        state, bd = np.zeros(self.src.size, dtype=np.uint32), np.zeros((self.src.size, G), dtype=np.float32)
        op, tl = np.zeros((self.src.size, G), dtype=bool), np.zeros((self.src.size, tiles), dtype=bool)
        for c in range(self.src.size):
            s, h = int(self.src[c]), int(hold[c])
            w = h | OPEN
            k = sql.bin_stated(int(self.fcw[c]), logn)
            for g in range(G):
                jg = slot_frames_stated(J, g)
                bd[c, g] = sql.band_stated(rows[s, g], k, self.B)
                with np.errstate(all="ignore"):
                    w = sql.step_stated(h, bd[c, g], np.float32(self.open[s] * np.float32(jg)), np.float32(self.close[s] * np.float32(jg)), self.hang, jg)
                h, op[c, g] = w & ~OPEN, bool(w & OPEN)
            state[c] = w
            for t in range(tiles):
                tl[c, t] = tile_open_stated(op[c], first, hop, self.lead, *tile_span_stated(t, TO, T, W))
        return state, bd, op, tl


class Feed:
    """The tile-squelched host form of a feed of one of the three tuners: tuners[c] is channel c's host form on its source's rows, data[S] the whole source
    rows, N / hop / win the spectrum, TO the tuner's outputs per tile.  block(a, b) takes the source samples a .. b - 1: the slots' rows, the decisions (when a
    SlotSquelch is set), every channel's unsquelched block from its current carry — the histories and counts go on whatever the decision; a tile that is
    not the block's first does not depend on its neighbours — and, for a closed tile, +0 for y and p, with a zero carry where it holds the last output."""

    def __init__(self, tuners, source, data, N, hop, TO, win=None):
        self.tuners, self.src, self.data, self.N, self.hop, self.TO, self.win = list(tuners), list(source), data, int(N), int(hop), int(TO), win
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
        """-> (Y float32 [C][T], P float32 [C][T], U float32 [C][T] the unsquelched y from the same carry, and (state, bands, open, mask, tiles, J) or None)."""
        n = len(self.tuners) if channels is None else int(channels)
        got = [slot_rows(self.data[s][a:b], self.N, self.hop, self.win, self.count) for s in range(len(self.data))]
        rows, J, first = np.stack([g[0] for g in got]), got[0][1], got[0][2]
        Y, P, U, dec, flags = [], [], [], None, None
        for c in range(len(self.tuners)):   # (the channels beyond the launch's keep their carry; their source's history goes on)
            t = self.tuners[c]
            if c >= n:
                keep = t.carry.copy()
                t.block(self.data[self.src[c]][a:b])
                t.carry[:] = keep
                continue
            y, z = t.block(self.data[self.src[c]][a:b], want_z=True)
            p = ml.power(z)
            if self.squelch is not None and dec is None:
                state, bd, op, mask, tiles = self.squelch.block(rows, J, first, self.hop, self.TO, y.size, b - a, n)
                dec, flags = (state, bd, op, mask, tiles, J), unpack(mask, tiles)
            U.append(y.copy())
            if flags is not None:
                y, p = y.copy(), p.copy()
                for k in np.flatnonzero(~flags[c]):
                    y[k * self.TO:(k + 1) * self.TO] = 0
                    p[k * self.TO:(k + 1) * self.TO] = 0
                if not flags[c, -1]:
                    t.carry[:] = 0
            Y.append(y)
            P.append(p)
        self.count += b - a
        return np.stack(Y), np.stack(P), np.stack(U), dec
