"""Transmitters whose symbol clock is off (TEST INFRASTRUCTURE ONLY, numpy only): the test generator (oracle/m17_oracle_gen.hpp) places one
symbol per 10 samples exactly, so transmitter and receiver share one clock.  resample_clock() re-reads such a signal at (1 + ppm * 1e-6)
times the nominal rate through a Hann-windowed sinc; the oracle and the library under test are then fed the SAME int16 array, so the
interpolation's fidelity is beside the point: it is deterministic, the result still decodes, and the receiver's clock recovery has to move."""
import concurrent.futures
import os

import numpy as np

import oracle_lib as ol

THREADS = min(16, os.cpu_count() or 1)

# the grid the GPU tests draw from: near the clock (the Kalman estimate leaves zero, sample_index hardly moves), the range in which every
# frame still decodes while sample_index moves 19-47 times in 96 000 samples (200 .. 800), and the range in which sync is lost and regained
PPM_GRID = (0, 20, -20, 60, -60, 200, -200, 500, -500, 800, -800, 1000, -1000, 2000)
MAX_PPM = 2000


def par(fn, items):
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(fn, items))


def resample_clock(x, ppm, half=16):
    """out[n] = sum over k in (-half, half] of x[floor(p) + k] * sinc(f - k) * hann(f - k), p = n (1 + ppm 1e-6), f = p - floor(p),
    hann(d) = 0.5 (1 + cos(pi d / half)) for |d| < half (else 0): in float64, samples outside the array are 0, rounded to nearest-even and
    saturated to int16.  x: int16, [T] with one ppm or [C][T] with one ppm per row (a scalar serves every row).  ppm = 0 returns x."""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim in (1, 2)
    if x.ndim == 2:
        pp = np.broadcast_to(np.asarray(ppm, dtype=np.float64), (x.shape[0],))
        return np.stack(par(lambda c: resample_clock(x[c], float(pp[c]), half), range(x.shape[0]))) if x.shape[0] else x.copy()
    T = x.size
    p = np.arange(T, dtype=np.float64) * (1.0 + float(ppm) * 1e-6)
    i0 = np.floor(p)
    f = p - i0
    i0 = i0.astype(np.int64)
    pad = half + int(np.ceil(T * abs(float(ppm)) * 1e-6)) + 2
    xp = np.zeros(T + 2 * pad, dtype=np.float64)
    xp[pad:pad + T] = x
    acc = np.zeros(T, dtype=np.float64)
    for k in range(-half + 1, half + 1):
        d = f - k
        w = np.sinc(d) * np.where(np.abs(d) < half, 0.5 * (1.0 + np.cos(np.pi * d / half)), 0.0)
        acc += xp[np.clip(i0 + k + pad, 0, xp.size - 1)] * w
    return np.clip(np.rint(acc), -32768.0, 32767.0).astype(np.int16)


def burst(seed, kind, T, sigma=300.0, ppm=0.0, n_frames=None, **kw):
    """One channel of T samples: loud noise, then ONE transmission of `kind` that fills the rest of the stream, sent by a transmitter `ppm` off.
    The generator makes enough samples for the fastest transmitter of the grid, so no sample of the result comes from outside its array."""
    n = T + int(np.ceil(T * MAX_PPM * 1e-6)) + 64
    nf = T // 1920 - 6 if n_frames is None else n_frames
    p = ol.gen_params(seed=seed, kind=kind, n_frames=nf, lead_in=3072, noise_sigma=sigma, tail_sigma=max(sigma, 100.0), lead_sigma=40000.0, total=n, **kw)
    return resample_clock(ol.generate(p)[:n], ppm)[:T].copy()


_BATCHES = {}


def batch(C, T, seeds, kinds=(0, 1, 2, 4), sigmas=(0.0, 300.0, 1200.0), grid=PPM_GRID):
    """C channels x T samples, cached per (arguments): channel c is burst() of seed seeds[c], kind kinds[c % len], noise sigmas[(c // len(kinds)) % len] and
    ppm grid[c % len(grid)] — with 4 kinds, 3 noise levels and 14 ppm values the combinations walk through one another, and a batch of 64
    holds every ppm value 4 or 5 times.  Returns a dict: x [C][T] int16 (read-only), ppm, kind, sigma (per channel), twin() -> the same
    channels sent on the clock (made when first asked for)."""
    seeds = tuple(int(v) for v in seeds)
    assert len(seeds) >= C
    key = (C, T, seeds[:C], tuple(kinds), tuple(sigmas), tuple(grid))
    if key not in _BATCHES:
        ppm = np.array([grid[c % len(grid)] for c in range(C)], dtype=np.float64)
        kind = np.array([kinds[c % len(kinds)] for c in range(C)])
        sigma = np.array([sigmas[(c // len(kinds)) % len(sigmas)] for c in range(C)])
        x = np.stack(par(lambda c: burst(seeds[c], int(kind[c]), T, float(sigma[c]), float(ppm[c])), range(C)))
        for a in (x, ppm, kind, sigma):
            a.setflags(write=False)
        made = {}

        def twin():
            if "x" not in made:
                made["x"] = np.stack(par(lambda c: burst(seeds[c], int(kind[c]), T, float(sigma[c]), 0.0), range(C)))
                made["x"].setflags(write=False)
            return made["x"]
        _BATCHES[key] = dict(x=x, twin=twin, ppm=ppm, kind=kind, sigma=sigma)
    return _BATCHES[key]


def scenarios(seed, C, T=96000, grid=PPM_GRID):
    """C channels of oracle_lib.random_scenario (seeds seed * 1000 + c; its defaults untouched), each re-read at a ppm drawn from the grid.
    Returns (x [C][T], ppm [C]); cached."""
    key = ("scenarios", seed, C, T, tuple(grid))
    if key not in _BATCHES:
        rng = np.random.default_rng(seed)
        ppm = rng.choice(np.asarray(grid, dtype=np.float64), C)
        n = T + int(np.ceil(T * MAX_PPM * 1e-6)) + 64
        x = np.stack(par(lambda c: resample_clock(ol.random_scenario(seed * 1000 + c, total=n), float(ppm[c]))[:T], range(C)))
        x.setflags(write=False)
        _BATCHES[key] = (x, ppm)
    return _BATCHES[key]


def index_moves(log):
    """Changes of sample_index between consecutive entries of one channel's diagnostic log."""
    si = np.asarray(log["sample_index"])
    return int((si[1:] != si[:-1]).sum())


def lost_and_regained(log):
    """True when `locked` goes 1 -> 0 -> 1 somewhere in the log."""
    lk = np.asarray(log["locked"]) != 0
    if not lk.any():
        return False
    first = int(np.argmax(lk))
    rest = lk[first:]
    if rest.all():
        return False
    gap = first + int(np.argmin(rest))
    return bool(lk[gap:].any())


# ---- the inputs of tests/test_gpu_off_clock.py, named here so that tests/test_off_clock.py asserts its conditions on exactly these ----------
MAIN_C, MAIN_T = 64, 96000
# per-channel generator seeds 9100 + 7 c; four channels take the next candidate (+ 1000): with the first one the ORACLE loses the transmission
# for reasons of its own (their on-clock twins do too), and the conditions of tests/test_off_clock.py are about the clock, checked on every channel
MAIN_SEEDS = tuple(9100 + 7 * c + (1000 if c in (7, 34, 36, 52) else 0) for c in range(MAIN_C))
# channel polarity table of the mixed-polarity case (and which transmitters are inverted for it)
POLARITY = tuple(int(v) for v in np.random.default_rng(640).integers(0, 2, MAIN_C))
# channels that get fresh demodulators between the two runs of the reset case: every |ppm| of the grid, both signs, every kind
RESET_CHANNELS = (0, 1, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 21, 22, 35, 40, 50, 63)
SCENARIO_SEEDS = (11, 22, 33)
KALMAN_ORDERS = (0, 1, 2, 3, 7)


def main():
    return batch(MAIN_C, MAIN_T, MAIN_SEEDS)


def negated(x):
    """The same transmissions from an inverted transmitter (-32768 has no opposite: it saturates)."""
    return np.clip(-x.astype(np.int32), -32768, 32767).astype(np.int16)


def main_mixed_polarity():
    """main()'s channels, those with POLARITY[c] = 1 negated."""
    key = "mixed_polarity"
    if key not in _BATCHES:
        x = main()["x"]
        pol = np.array(POLARITY, dtype=np.uint8)
        y = np.where(pol[:, None] == 1, negated(x), x)
        y.setflags(write=False)
        _BATCHES[key] = (y, pol)
    return _BATCHES[key]


def bursty(seed=5500, C=32, T=96000):
    """Short transmissions of every kind, each from a transmitter +500 or -500 ppm off, between stretches of loud, quiet and no noise (the input
    of the gate-aware front end's test, tests/test_gpu_parity.py, shortened): the carrier detect closes by forced unlocks and reopens on the next
    preamble while the clock of each transmission drifts.  Returns (x [C][T], ppm of the first burst per channel); cached."""
    key = ("bursty", seed, C, T)
    if key not in _BATCHES:
        rng = np.random.default_rng(seed)
        plans = []
        for c in range(C):
            pos, plan = 0, []
            while pos < T - 9000:
                n = min(int(rng.integers(9000, 40000)), T - pos)
                kw = dict(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.choice([0, 1, 2, 4])), n_frames=int(rng.integers(2, 12)),
                          lead_in=int(rng.integers(0, 6000)), lead_sigma=float(rng.choice([100.0, 20000.0, 40000.0])),
                          noise_sigma=float(rng.choice([100.0, 600.0, 1500.0])), tail_sigma=float(rng.choice([100.0, 5000.0, 20000.0])),
                          phase=int(rng.integers(-1, 10)))
                plan.append((pos, n, kw, float(rng.choice([500.0, -500.0]))))
                pos += n
            plans.append((plan, pos, rng.integers(-300, 300, T - pos).astype(np.int16)))

        def make(c):
            plan, end, rest = plans[c]
            row = np.zeros(T, dtype=np.int16)
            for pos, n, kw, ppm in plan:
                row[pos:pos + n] = resample_clock(ol.generate(ol.gen_params(total=n + 128, **kw))[:n + 128], ppm)[:n]
            row[end:] = rest
            return row
        x = np.stack(par(make, range(C)))
        x.setflags(write=False)
        _BATCHES[key] = (x, np.array([p[0][0][3] for p in plans]))
    return _BATCHES[key]


_ORACLE = {}


def oracle_of(name, x, invert=None, logs=False):
    """The oracle over x [C][T], channel c under polarity invert[c] (None: plain), cached under `name`: rows (the records per channel),
    diags [C], and (logs) every diagnostic callback per channel."""
    key = (name, logs)
    if key not in _ORACLE:
        C, T = x.shape
        inv = np.zeros(C, dtype=np.uint8) if invert is None else np.asarray(invert, dtype=np.uint8)
        rows, diags = [None] * C, np.zeros(C, dtype=ol.DIAG)
        for v in (0, 1):
            chs = np.flatnonzero(inv == v)
            if not chs.size:
                continue
            recs, counts, d = ol.demod_batch(np.ascontiguousarray(x[chs]), invert=v, cap=2 * (T // 1920 + 2) + 4, threads=THREADS)
            for i, c in enumerate(chs):
                rc = recs[i, : counts[i]].copy()
                rc["channel"] = c
                rows[c], diags[c] = rc, d[i]
        lg = par(lambda c: demod_log(x[c], int(inv[c])), range(C)) if logs else None
        _ORACLE[key] = (rows, diags, lg)
    return _ORACLE[key]


def demod_log(x, invert=0):
    return ol.demod_diag_log(np.ascontiguousarray(x), invert=invert, cap=x.size // 384 + 2)


def log_pos(log):
    """The sample (since the demodulator's start) whose processing fired each callback of a log."""
    return log["pad"][:, 0].astype(np.uint64) | (log["pad"][:, 1].astype(np.uint64) << np.uint64(32))


def locked_moves(log):
    """Changes of sample_index between consecutive log entries that are both locked: moves of a running transmission, not acquisitions."""
    si, lk = np.asarray(log["sample_index"]), np.asarray(log["locked"]) != 0
    return int(((si[1:] != si[:-1]) & lk[1:] & lk[:-1]).sum())
