"""The FLOAT oracle (tests/cxx/f32_oracle.cpp): the oracle's demodulator stepped on float32 samples in the reference's units — what
M17Demodulator<float>::operator()(float) receives — and the signals the float-input tests share.

TEST INFRASTRUCTURE ONLY, like oracle_lib: built on first use with g++ -O2 -ffp-contract=off and loaded through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "f32_oracle.cpp")
LIB = os.path.join(ROOT, "tests", "cxx", "libf32oracle.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(ol.ORACLE_DIR, f) for f in os.listdir(ol.ORACLE_DIR) if f.endswith((".hpp", ".inc"))]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = LIB + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        _lib.f32o_demod.restype = C.c_size_t
        _lib.f32o_diag_log.restype = C.c_size_t
    return _lib


def _f32(x):
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x


def demod(x, invert=0, cap=4096):
    """Records and the last m17_diag of one channel of floats."""
    x = _f32(x)
    recs = np.zeros(cap, dtype=ol.FRAME_REC)
    diag = np.zeros(1, dtype=ol.DIAG)
    n = lib().f32o_demod(ol._p(x), C.c_size_t(x.size), C.c_int(invert), ol._p(recs), C.c_size_t(cap), ol._p(diag))
    assert n <= cap
    return recs[:n].copy(), diag[0].copy()


def diag_log(x, invert=0, cap=4096):
    """Every diagnostic callback of one channel of floats (the layout of m17hip_diag_log_fetch / ol.demod_diag_log)."""
    x = _f32(x)
    log = np.zeros(cap, dtype=ol.DIAG)
    n = lib().f32o_diag_log(ol._p(x), C.c_size_t(x.size), C.c_int(invert), ol._p(log), C.c_size_t(cap))
    assert n <= cap
    return log[:n].copy()


def demod_batch(x, invert=None, threads=16, logs=False):
    """x[C][T] float32; invert: None, 0 / 1, or one entry per channel.  Returns (recs[C][cap], counts[C], diags[C]) and, with logs, (log[C][lcap],
    log_counts[C]) as well."""
    x = _f32(x)
    Cn, T = x.shape
    cap = 2 * (T // 1920 + 2) + 4
    lcap = T // 384 + 2
    inv = None
    if invert is not None:
        inv = np.ascontiguousarray(np.broadcast_to(np.asarray(invert, dtype=np.uint8), (Cn,)))
    recs = np.zeros((Cn, cap), dtype=ol.FRAME_REC)
    counts = np.zeros(Cn, dtype=np.uint32)
    diags = np.zeros(Cn, dtype=ol.DIAG)
    lg = np.zeros((Cn, lcap), dtype=ol.DIAG) if logs else None
    lc = np.zeros(Cn, dtype=np.uint32) if logs else None
    lib().f32o_demod_batch(ol._p(x), C.c_size_t(Cn), C.c_size_t(T), C.c_size_t(T), None if inv is None else ol._p(inv), C.c_int(threads), ol._p(recs),
                           C.c_size_t(cap), ol._p(counts), ol._p(diags), None if lg is None else ol._p(lg), C.c_size_t(lcap),
                           None if lc is None else ol._p(lc))
    assert (counts <= cap).all() and (lc is None or (lc <= lcap).all())
    return (recs, counts, diags, lg, lc) if logs else (recs, counts, diags)


# ---- the signals ----------------------------------------------------------------------------------------------------------------------------
def on_grid(s):
    """float(double(s) / 41067.0): what apps/m17-demod.cpp:489 hands the reference for the int16 sample s."""
    return (np.asarray(s, dtype=np.float64) / 41067.0).astype(np.float32)


def off_grid(s, seed):
    """Floats that are NOT int16 / 41067: 0.37 (s + u) / 41067 + 0.0123 with u uniform in +-0.5 — another gain, a DC offset, no quantisation."""
    s = np.asarray(s)
    u = np.random.default_rng(seed).uniform(-0.5, 0.5, size=s.shape)
    return (0.37 * (s.astype(np.float64) + u) / 41067.0 + 0.0123).astype(np.float32)


def times4(s):
    """4 x the nominal amplitude: most samples lie beyond +-32767 / 41067, where an int16 host saturates."""
    return (4.0 * np.asarray(s, dtype=np.float64) / 41067.0).astype(np.float32)


def round_trip(x):
    """What the int16 path made of a float: lrint(x * 41067), saturated to int16."""
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 41067.0), -32768, 32767).astype(np.int16)


def survives_round_trip(x):
    return on_grid(round_trip(x)).view(np.uint32) == np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
