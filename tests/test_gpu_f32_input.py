"""GPU tests of float32 baseband input (ABI 607, include/m17hip.h: m17hip_upload_f32 and friends).  A float stream's samples are what the reference's
M17Demodulator<float>::operator() receives; every kernel that reads the input has a float form.  Every comparison is exact — float tables as uint32
words, records, m17_diag and the diagnostic log byte for byte — against the oracle's operators (m17o_fir_f32, m17o_dcd_sums) and against the float
oracle (tests/cxx/f32_oracle.cpp: the oracle's demodulator stepped on those floats).  The premises (off-grid floats and floats beyond int16 change what
a rounding host gets) are asserted on the oracle alone in tests/test_f32_input.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
THREADS = 16
INV = m17hip.FLAG_INVERT
INT_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _neg(x):
    """Negation as a float stream does it: the sign bit flipped (NaNs, zeroes and denormals included)."""
    return (_u32(x) ^ np.uint32(0x80000000)).view(np.float32)


def _spice(x, rng):
    """Values beyond +-1, denormals of magnitude 1e-40 and -0.0 sprinkled over every row."""
    x = x.copy()
    n = x.shape[-1]
    for row in x.reshape(-1, n):
        k = max(1, n // 9)
        row[rng.integers(0, n, k)] = rng.uniform(-7.0, 7.0, k).astype(np.float32)
        row[rng.integers(0, n, k)] = np.float32(1e-40) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), k)
        row[rng.integers(0, n, k)] = np.float32(-0.0)
    return x


# ---- 1: K1, one hop ----------------------------------------------------------------------------------------------------------------------------
FIR_C, FIR_TS = (1, 3, 65), (7, 31, 4095, 4096, 4097, 8193)


@pytest.fixture(scope="module")
def fir_case():
    rng = np.random.default_rng(607)
    T = max(FIR_TS)
    x = _spice(rng.uniform(-1.0, 1.0, size=(max(FIR_C), T)).astype(np.float32), rng)
    assert (np.abs(x) > 1).any() and (x == 0).any() and ((x != 0) & (np.abs(x) < 1e-38)).any()
    # y[t] depends on x[0 .. t] alone: the expectation of a shorter slab is a prefix of the longest one's
    exp = np.stack([np.stack([ol.fir_f32(x[c]), ol.fir_f32(_neg(x[c]))]) for c in range(max(FIR_C))])   # [c][polarity][t]
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("Cn", FIR_C)
def test_matched_filter_on_float_rows(fir_case, Cn, grid):
    """m17hip_fir_rrc150 on a float stream against m17o_fir_f32, bit for bit: tile edges and the end of the slab inside a chunk, one and two workgroups
    (key 13: one workgroup walks several items), uniform plain, uniform inverted and items of alternating polarity."""
    x, exp = fir_case
    ctx = m17hip.Context(max(FIR_C), max(FIR_TS))
    try:
        ctx.tune(13, grid)
        for T in FIR_TS:
            ctx.reset()
            ctx.upload(x[:Cn, :T])
            assert ctx.download_f32().tobytes() == np.ascontiguousarray(x[:Cn, :T]).tobytes()
            for pol in (None, (np.arange(Cn) & 1).astype(np.uint8)):
                if pol is not None and Cn == 1:
                    continue
                ctx.set_channel_polarity(pol)
                for flag in (0, INV):
                    y = ctx.fir(flags=flag)
                    for c in range(Cn):
                        p = (0 if pol is None else int(pol[c])) ^ (1 if flag else 0)
                        e = exp[c, p, :T]
                        assert np.array_equal(_u32(y[c]), _u32(e)), (T, Cn, grid, flag, c, int(np.flatnonzero(_u32(y[c]) != _u32(e))[0]))
            ctx.set_channel_polarity(None)
    finally:
        ctx.close()


# ---- 2: K3, both forms, one hop ----------------------------------------------------------------------------------------------------------------
DCD_CMAX, DCD_TMAX = 65, 1000


@pytest.fixture(scope="module")
def table_case():
    rng = np.random.default_rng(20261018)
    x = _spice(rng.uniform(-1.0, 1.0, size=(DCD_CMAX, DCD_TMAX)).astype(np.float32), rng)
    ticks = DCD_TMAX // 192
    exp = np.zeros((2, DCD_CMAX, ticks, 2, 6), dtype=np.float32)
    for inv in (0, 1):
        for c in range(DCD_CMAX):
            xs = _neg(x[c]) if inv else x[c]
            for k in range(ticks):
                for j in range(6):
                    a0 = 0 if j == 5 else max(k - ((k - j) % 5), 0)   # sum j restarts with the ticks = j (mod 5); sum 5 runs from the stream start
                    exp[inv, c, k, :, j] = ol.dcd_sums(xs, 192 * a0, 192 * (k - a0 + 1))
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


def _dcd_patterns(Cn):
    rng = np.random.default_rng(17 + Cn)
    return {"uniform": None, "alternating": (np.arange(Cn) & 1).astype(np.uint8), "random": rng.integers(0, 2, Cn).astype(np.uint8)}


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("Cn", [1, 33, 65])
def test_carrier_detect_table_on_float_rows(table_case, Cn, form):
    x, exp = table_case
    ctx = m17hip.Context(DCD_CMAX, DCD_TMAX)
    try:
        ctx.tune(10, form)
        for name, pol in _dcd_patterns(Cn).items():
            ctx.set_channel_polarity(pol)
            for T in (31, 192, 193, 960, 1000):
                ctx.reset()
                ctx.upload(x[:Cn, :T])
                for flag in (0, INV):
                    sums = ctx.dcd(flags=flag)
                    eff = (np.zeros(Cn, dtype=np.uint8) if pol is None else pol) ^ (1 if flag else 0)
                    e = np.stack([exp[eff[c], c, : T // 192] for c in range(Cn)])
                    assert sums.shape == e.shape
                    bad = np.flatnonzero((_u32(sums) != _u32(e)).reshape(Cn, -1).any(axis=1))
                    assert bad.size == 0, (name, T, flag, bad[:16].tolist())
    finally:
        ctx.close()


# ---- the full chain ----------------------------------------------------------------------------------------------------------------------------
CH_C, CH_T = 64, 96000
KW = dict(seed=6040, kind=-1, n_frames=CH_T // 1920 - 6, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=CH_T)


class Expect:
    """The float oracle over whole streams x[C][T] (channel c under invert[c], from sample origin[c] on): records and log entries of the run that
    covers samples [b0, b1) of the context's stream, and m17_diag at the end of the stream."""

    def __init__(self, x, invert=None, origin=None):
        self.C, self.T = x.shape
        self.origin = np.zeros(self.C, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
        self.recs, self.logs, self.diags = [None] * self.C, [None] * self.C, np.zeros(self.C, dtype=ol.DIAG)
        inv = np.zeros(self.C, dtype=np.uint8) if invert is None else np.broadcast_to(np.asarray(invert, dtype=np.uint8), (self.C,))
        for a in np.unique(self.origin):
            chs = np.flatnonzero(self.origin == a)
            r, n, d, lg, ln = fl.demod_batch(np.ascontiguousarray(x[chs, a:]), invert=inv[chs], threads=THREADS, logs=True)
            for i, c in enumerate(chs):
                self.recs[c] = r[i, : n[i]].copy()
                self.recs[c]["channel"] = c
                self.logs[c] = lg[i, : ln[i]].copy()
                self.diags[c] = d[i]

    def run(self, b0, b1):
        rows, logs = [], []
        for c in range(self.C):
            lo, hi = b0 - self.origin[c], b1 - self.origin[c]
            r = self.recs[c]
            r = r[(r["sample_pos"] >= max(lo, 0)) & (r["sample_pos"] < hi)].copy()
            rows.append(r)
            lg = self.logs[c]
            pos = lg["pad"][:, 0].astype(np.int64) | (lg["pad"][:, 1].astype(np.int64) << 32)
            logs.append(lg[(pos >= max(lo, 0)) & (pos < hi)])
        return rows, logs


def _check(ctx, rows, logs, what, diags=None, got=None):
    Cn = len(rows)
    got = ctx.frames().copy() if got is None else got
    e = np.concatenate(rows)
    if got.tobytes() != e.tobytes():
        bad = [c for c in range(Cn) if got[got["channel"] == c].tobytes() != rows[c].tobytes()]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {e.size} expected), channels {bad[:24]}")
    if logs is not None:
        glog = ctx.diag_log(Cn, capacity=CH_T // 384 + 2)
        for c in range(Cn):
            assert glog[c].tobytes() == logs[c].tobytes(), (what, "diagnostic log", c, glog[c].size, logs[c].size)
    if diags is not None:
        d = ctx.diag(Cn)
        for f in INT_FIELDS:
            assert np.array_equal(d[f], diags[f]), (what, f, np.flatnonzero(d[f] != diags[f])[:16].tolist())
        for f in FLOAT_FIELDS:
            assert np.array_equal(d[f], diags[f], equal_nan=True), (what, f)


def _ctx(Cn, T, knobs=None, log=True):
    ctx = m17hip.Context(Cn, T)
    for k, v in (knobs or {}).items():
        ctx.tune(k, v)
    if log:
        ctx.tune(9, CH_T // 384 + 2)
    return ctx


@pytest.fixture(scope="module")
def base():
    s = ol.generate_batch(ol.gen_params(invert=0, **KW), CH_C, CH_T, threads=THREADS)
    s.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def off_case(base):
    x = fl.off_grid(base, seed=607)
    assert fl.survives_round_trip(x).mean() < 0.01
    exp = Expect(x)
    assert all(r.size > 6 for r in exp.recs), "every channel yields frames"
    x.setflags(write=False)
    return x, exp


@pytest.fixture(scope="module")
def x4_case(base):
    x = fl.times4(base)
    assert (np.abs(x) > 32767.0 / 41067.0).mean() > 0.3
    exp = Expect(x)
    assert all(r.size > 6 for r in exp.recs)
    x.setflags(write=False)
    return x, exp


def test_int16_derived_floats_equal_the_int16_path(base):
    """On float(double(s) / 41067.0) a float stream gives what the int16 path of the same build gives on s: records, m17_diag, diagnostic log."""
    ctx = _ctx(CH_C, CH_T)
    try:
        out = []
        for data in (base, fl.on_grid(base)):
            ctx.reset()
            ctx.upload(data)
            ctx.run()
            out.append((ctx.frames().tobytes(), ctx.diag(CH_C).tobytes(), b"".join(l.tobytes() for l in ctx.diag_log(CH_C, capacity=CH_T // 384 + 2))))
        assert len(out[0][0]) > 64 * CH_C and out[0] == out[1]
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["off_grid", "times4"])
@pytest.mark.parametrize("knobs", [{}, {3: 4800}, {10: 0}, {20: 1}, {15: 0, 17: 0}], ids=["default", "seg4800", "one_wave_dcd", "redo_in_front", "decode_and_evm_in_k5"])
def test_full_chain_equals_the_float_oracle(off_case, x4_case, which, knobs):
    x, exp = off_case if which == "off_grid" else x4_case
    ctx = _ctx(CH_C, CH_T, knobs)
    try:
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        rows, logs = exp.run(0, CH_T)
        _check(ctx, rows, logs, f"{which} {knobs}", diags=exp.diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("cuts", ["ragged", "runs_of_1927"])
def test_full_chain_in_ragged_runs(off_case, cuts):
    """A continued float stream in place: ragged segments (no multiple of 8, 32 or 192) and runs of 1927 samples — the carried float prefix, the
    sample-by-sample head and tail of the carrier detect, the patch windows of K2 and K5 across runs."""
    x, exp = off_case
    Cn = 16
    if cuts == "ragged":
        b = [0, 4801, 4801 + 19203, 50001, 50001 + 7, 71111, CH_T]
    else:
        b = list(range(0, 1927 * 12, 1927)) + [CH_T]
    ctx = _ctx(Cn, CH_T)
    try:
        ctx.reset()
        for r in range(len(b) - 1):
            ctx.upload(x[:Cn, b[r]:b[r + 1]])
            ctx.run()
            rows, logs = exp.run(b[r], b[r + 1])
            last = r + 2 == len(b)
            _check(ctx, rows[:Cn], logs[:Cn], f"{cuts}, run {r}", diags=exp.diags[:Cn] if last else None)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["front_then_run", "run_only"])
def test_full_chain_staged_live_feed(x4_case, order):
    """stage; front; run; frames_select(1); fetch — and the same without the front call: float slabs alternate, the float tail is carried across."""
    import torch
    x, exp = x4_case
    n_runs, T = 4, CH_T // 4
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(n_runs)]
    ctx = _ctx(CH_C, T, log=False)
    try:
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), CH_C, T, dtype=np.float32)
        ctx.run(channels=CH_C, samples=T)
        for r in range(n_runs):
            if r + 1 < n_runs:
                ctx.upload_async(pins[r + 1].data_ptr(), CH_C, T, dtype=np.float32)
                if order == "front_then_run":
                    ctx.front(channels=CH_C, samples=T)
                ctx.run(channels=CH_C, samples=T)
                ctx.frames_select(1)
            got = ctx.frames().copy()
            ctx.frames_select(0)
            rows, _ = exp.run(r * T, (r + 1) * T)
            _check(ctx, rows, None, f"live feed {order}, run {r}", diags=exp.diags if r + 1 == n_runs else None, got=got)
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


def test_staged_float_runs_shorter_than_the_prefixes_mixed_with_in_place_runs(off_case):
    """The float form of test_gpu_streaming's ragged mixed staging: runs shorter than the carried prefixes (152 input samples, 96 filter outputs), no
    multiples of 8 / 192 / 1920, in place / staged with m17hip_demod_front / staged without it in turn, up to one frame cycle past the last cut.  A staged
    float run finds its prefix in the previous run's prefix (a run shorter than 152 samples) or in that run's tail where it lies."""
    import torch
    x, exp = off_case
    Cn = 16
    cuts = [1, 7, 95, 149, 153, 1919, 3841, 1920]   # (the last: one frame cycle)
    end = sum(cuts)
    diags = Expect(np.ascontiguousarray(x[:Cn, :end])).diags
    ctx = _ctx(Cn, CH_T, log=False)
    try:
        ctx.reset()
        pos, keep, total = 0, [], 0
        for i, n in enumerate(cuts):
            chunk = np.ascontiguousarray(x[:Cn, pos:pos + n])
            if i % 3 == 0:                             # in place
                ctx.upload(chunk)
                ctx.run()
            else:
                pin = torch.from_numpy(chunk).pin_memory()
                keep.append(pin)
                ctx.upload_async(pin.data_ptr(), Cn, n, dtype=np.float32)
                if i % 3 == 1:
                    ctx.front(channels=Cn, samples=n)
                ctx.run(channels=Cn, samples=n)
            rows, _ = exp.run(pos, pos + n)
            last = i + 1 == len(cuts)
            _check(ctx, rows[:Cn], None, f"run {i} of {n} samples", diags=diags if last else None)
            total += sum(r.size for r in rows[:Cn])
            pos += n
        ctx.upload_wait()
        assert pos == end and total > 0
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


def test_staged_float_run_after_an_in_place_overwrite_of_the_previous_slab(off_case):
    """The float form of test_gpu_streaming's test of that name: a run in place, then the same slab overwritten in place (an input that is never run),
    then the NEXT chunk staged and run: the staged run's 152-sample prefix must be the tail the last RUN carried, not what the data region holds now."""
    import torch
    x, exp = off_case
    Cn, T = 16, 9600
    diags = Expect(np.ascontiguousarray(x[:Cn, :2 * T])).diags
    junk = np.full((Cn, T), 0.3, dtype=np.float32)
    pinned = torch.from_numpy(np.ascontiguousarray(x[:Cn, T:2 * T])).pin_memory()
    ctx = _ctx(Cn, CH_T, log=False)
    try:
        ctx.reset()
        ctx.upload(x[:Cn, :T])
        ctx.run(channels=Cn, samples=T)
        rows, _ = exp.run(0, T)
        _check(ctx, rows[:Cn], None, "the run in place")
        total = sum(r.size for r in rows[:Cn])
        ctx.upload(junk)                                                   # overwrites the slab the run used (never run)
        ctx.upload_async(pinned.data_ptr(), Cn, T, dtype=np.float32)       # the real continuation, staged
        ctx.run(channels=Cn, samples=T)
        rows, _ = exp.run(T, 2 * T)
        _check(ctx, rows[:Cn], None, "the staged continuation", diags=diags)
        total += sum(r.size for r in rows[:Cn])
        ctx.upload_wait()
        assert total > Cn
    finally:
        ctx.close()


@pytest.mark.parametrize("order", range(8))
def test_every_kalman_order(off_case, order):
    x, _ = off_case
    Cn, T = 8, 48000
    xs = np.ascontiguousarray(x[:Cn, :T])
    try:
        fl.lib().f32o_set_kalman_order(C.c_int(order))
        exp = Expect(xs)
    finally:
        fl.lib().f32o_set_kalman_order(C.c_int(3))
    ctx = _ctx(Cn, T)
    try:
        ctx.set_kalman_order(order)
        ctx.upload(xs)
        ctx.reset()
        ctx.run()
        rows, logs = exp.run(0, T)
        assert sum(r.size for r in rows) > Cn
        _check(ctx, rows, logs, f"kalman order {order}", diags=exp.diags)
    finally:
        ctx.close()


def test_full_chain_mixed_polarity_table(base):
    """Rows of plain and inverted transmitters picked by a random pattern; the table is that pattern, the floats are off the int16 grid."""
    s1 = ol.generate_batch(ol.gen_params(invert=1, **KW), CH_C, CH_T, threads=THREADS)
    pol = np.random.default_rng(64).integers(0, 2, CH_C).astype(np.uint8)
    assert 16 < pol.sum() < 48
    x = fl.off_grid(np.where(pol[:, None] == 1, s1, base), seed=608)
    exp = Expect(x, invert=pol)
    assert all(r.size > 6 for r in exp.recs), "every channel yields frames under its own polarity"
    rows, logs = exp.run(0, CH_T)
    ctx = _ctx(CH_C, CH_T)
    try:
        ctx.set_channel_polarity(pol)
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        _check(ctx, rows, logs, "mixed table", diags=exp.diags)
        ctx.set_channel_polarity(pol ^ 1)   # (every channel's entry changes: all of them start over) and the flag turns them back
        ctx.upload(x)
        ctx.reset()
        ctx.run(flags=INV)
        _check(ctx, rows, logs, "mixed table, flagged", diags=exp.diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("gate", [0, 1])
def test_gate_aware_front_end_on_bursty_float_channels(gate):
    """Short transmissions between loud, quiet and no noise (tests/test_gpu_channel_polarity.py's bursty input) at 0.37 x the gain plus an offset: channels
    leave the limit-filter replay, K2 and K5 rebuild windows from the float input and the float snapshots, K1 skips what the carrier is off for."""
    Cn, T = 33, 240000
    x, exp = _bursty(Cn, T)
    rows, logs = exp.run(0, T)
    assert sum(r.size for r in rows) > Cn
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.tune(3, 4800)
        ctx.tune(26, gate)
        ctx.tune(9, T // 384 + 2)
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got = ctx.frames().copy()
        assert ctx.replay_drops() > 0
        glog = ctx.diag_log(Cn, capacity=T // 384 + 2)
        assert got.tobytes() == np.concatenate(rows).tobytes()
        for c in range(Cn):
            assert glog[c].tobytes() == logs[c].tobytes(), (c, glog[c].size, logs[c].size)
        d = ctx.diag(Cn)
        for f in INT_FIELDS:
            assert np.array_equal(d[f], exp.diags[f]), f
        for f in FLOAT_FIELDS:
            assert np.array_equal(d[f], exp.diags[f], equal_nan=True), f
    finally:
        ctx.close()


_bursty_cache = {}


def _bursty(Cn, T):
    if "x" not in _bursty_cache:
        rng = np.random.default_rng(5150)
        s = np.zeros((Cn, T), dtype=np.int16)
        for c in range(Cn):
            pos = 0
            while pos < T - 9000:
                n = min(int(rng.integers(9000, 70000)), T - pos)
                p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.choice([0, 1, 2, 4])), n_frames=int(rng.integers(1, 9)),
                                  lead_in=int(rng.integers(0, 6000)), lead_sigma=float(rng.choice([100.0, 20000.0, 40000.0])),
                                  noise_sigma=float(rng.choice([100.0, 600.0, 1500.0])), tail_sigma=float(rng.choice([100.0, 5000.0, 20000.0])),
                                  phase=int(rng.integers(-1, 10)), total=n)
                s[c, pos:pos + n] = ol.generate(p)[:n]
                pos += n
            s[c, pos:] = rng.integers(-300, 300, T - pos)
        x = fl.off_grid(s, seed=609)
        x.setflags(write=False)
        _bursty_cache["x"] = (x, Expect(x))
    return _bursty_cache["x"]


def test_reset_channels_between_float_runs(off_case):
    """Three runs of 19 200 samples; a third of the channels start over with the second run (on the tick grid).  Off the grid: M17HIP_ESTATE."""
    x, _ = off_case
    Cn, T, n_runs = 24, 19200, 3
    xs = np.ascontiguousarray(x[:Cn, : n_runs * T])
    again = np.arange(Cn)[::3]
    origin = np.zeros(Cn, dtype=np.int64)
    origin[again] = T
    exp = Expect(xs, origin=origin)
    ctx = _ctx(Cn, T)
    try:
        ctx.reset()
        for r in range(n_runs):
            if r == 1:
                ctx.reset_channels(again)
            ctx.upload(xs[:, r * T:(r + 1) * T])
            ctx.run()
            rows, logs = exp.run(r * T, (r + 1) * T)
            if r == 0:   # (before they start over, the channels concerned are channels like any other: from the stream's start)
                first = Expect(np.ascontiguousarray(xs[again, :T]))
                for i, c in enumerate(again):
                    rows[c], logs[c] = first.recs[i].copy(), first.logs[i]
                    rows[c]["channel"] = c
            _check(ctx, rows, logs, f"run {r}", diags=exp.diags if r + 1 == n_runs else None)
        ctx.upload(xs[:, :1000])
        ctx.run()
        assert ctx.lib.m17hip_demod_reset_channels(ctx.h, ol._p(np.array([0], dtype=np.uint32)), C.c_uint32(1)) == ESTATE
    finally:
        ctx.close()


# ---- the format belongs to the stream ----------------------------------------------------------------------------------------------------------
def _up(ctx, name, a):
    return getattr(ctx.lib, name)(ctx.h, ol._p(a), C.c_uint32(a.shape[0]), C.c_uint32(a.shape[1]), C.c_size_t(a.shape[1]))


def test_format_rule_and_refusals(base):
    Cn, T = 4, 9600
    s = np.ascontiguousarray(base[:Cn, :T])
    x = fl.off_grid(s, seed=1)
    ctx = m17hip.Context(Cn, T)
    try:
        assert ctx.input_format() == (0, 0)
        # argument refusals of the float entry points: null pointer, more than the context holds, pitch < samples
        for name in ("m17hip_upload_f32", "m17hip_upload_f32_async", "m17hip_upload_f32_device", "m17hip_upload_f32_device_async", "m17hip_download_f32"):
            fn = getattr(ctx.lib, name)
            assert fn(ctx.h, None, C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(T)) == EINVAL, name
            assert fn(ctx.h, ol._p(x), C.c_uint32(Cn + 1), C.c_uint32(T), C.c_size_t(T)) == EINVAL, name
            assert fn(ctx.h, ol._p(x), C.c_uint32(Cn), C.c_uint32(T + 1), C.c_size_t(T + 1)) == EINVAL, name
            assert fn(ctx.h, ol._p(x), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(T - 1)) == EINVAL, name
        assert ctx.input_format() == (0, 0)
        ctx.upload(x)
        fmt, nbytes = ctx.input_format()
        assert fmt == m17hip.FORMAT_F32 and nbytes >= Cn * T * 4
        assert ctx.download_f32().tobytes() == x.tobytes()
        out = np.zeros((Cn, T), dtype=np.int16)
        assert _up(ctx, "m17hip_download_i16", out) == ESTATE
        ctx.run()
        assert _up(ctx, "m17hip_upload_i16", s) == ESTATE            # an int16 upload on a float stream
        assert _up(ctx, "m17hip_upload_i16_async", s) == ESTATE
        p = ol.gen_params(seed=3, kind=1, n_frames=2, total=T)
        assert ctx.lib.m17hip_synth_i16(ctx.h, C.byref(p), C.c_uint32(Cn), C.c_uint32(T), C.c_uint32(0)) == ESTATE   # synthesis is int16
        ctx.upload(x)                                                # the stream goes on as it was
        ctx.run()
        ctx.reset()                                                  # frees the choice
        assert ctx.input_format()[0] == 0
        assert _up(ctx, "m17hip_upload_i16", s) == 0
        assert ctx.input_format()[0] == m17hip.FORMAT_I16
        assert _up(ctx, "m17hip_upload_f32", x) == ESTATE            # and the other way round
        assert _up(ctx, "m17hip_download_f32", np.zeros((Cn, T), dtype=np.float32)) == ESTATE
        ctx.run()
        assert ctx.download().tobytes() == s.tobytes()
    finally:
        ctx.close()


def test_a_context_that_never_sees_a_float_allocates_no_float_slab(base):
    Cn, T = 8, 19200
    s = np.ascontiguousarray(base[:Cn, :T])
    import torch
    pin = torch.from_numpy(s).pin_memory()
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.upload(s)
        ctx.reset()
        ctx.run()
        ctx.upload_async(pin.data_ptr(), Cn, T)   # (the second slab pair as well)
        ctx.run(channels=Cn, samples=T)
        ctx.frames()
        assert ctx.input_format() == (m17hip.FORMAT_I16, 0)
    finally:
        ctx.close()


# ---- non-finite samples ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_samples_stay_in_their_channel(off_case):
    x, exp = off_case
    Cn, T, bad = 8, 48000, 5
    ref = Expect(np.ascontiguousarray(x[:Cn, :T]))
    p = int(ref.recs[bad]["sample_pos"][1]) + 500   # two records of the poisoned channel lie before p
    assert p + 3000 < T
    xs = np.ascontiguousarray(x[:Cn, :T]).copy()
    xs[bad, p::3] = np.nan
    xs[bad, p + 1::3] = np.inf
    xs[bad, p + 2::3] = -np.inf
    ctx = _ctx(Cn, T)
    try:
        ctx.upload(xs)
        ctx.reset()
        assert ctx.lib.m17hip_demod_run(ctx.h, C.c_uint32(Cn), C.c_uint32(T), C.c_uint32(0)) == 0
        got = ctx.frames().copy()
        glog = ctx.diag_log(Cn, capacity=CH_T // 384 + 2)
        d = ctx.diag(Cn)
        for c in range(Cn):
            mine = got[got["channel"] == c]
            if c == bad:
                early = mine[mine["sample_pos"] < p]
                e = ref.recs[c][ref.recs[c]["sample_pos"] < p]
                assert e.size >= 2 and early.tobytes() == e.tobytes()
            else:
                assert mine.tobytes() == ref.recs[c].tobytes(), c
                assert glog[c].tobytes() == ref.logs[c].tobytes(), c
                for f in INT_FIELDS:
                    assert d[f][c] == ref.diags[f][c], (c, f)
    finally:
        ctx.close()


# ---- the GPU-backed M17Demodulator<float> ------------------------------------------------------------------------------------------------------
MIRROR_SRC = os.path.join(ROOT, "tests", "cxx", "f32_mirror_check.cpp")
MIRROR_EXE = os.path.join(ROOT, "tests", "cxx", "f32_mirror_check")


@pytest.fixture(scope="module")
def mirror_exe():
    if not os.path.exists(MIRROR_EXE) or os.path.getmtime(MIRROR_EXE) < os.path.getmtime(MIRROR_SRC):
        pkg = os.path.join(ROOT, "m17-cxx-demod_amd")
        subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(pkg, "include", "m17cxx"), MIRROR_SRC, "-L", pkg, "-lm17hip",
                        "-Wl,-rpath," + pkg, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", MIRROR_EXE], check=True)
    return MIRROR_EXE


@pytest.mark.parametrize("which", ["off_grid", "times4"])
def test_mirror_class_takes_floats_as_they_are(mirror_exe, base, tmp_path, which):
    """The GPU-backed M17Demodulator<float> fed floats that are no int16 / 41067 delivers the callback sequence of the scalar_cpu form on the same floats
    (it used to round them to int16, and to cast what lay beyond +-0.798 out of range)."""
    for c, kind in ((0, "a"), (1, "b"), (2, "c")):
        s = base[c, :38400]
        x = fl.off_grid(s, seed=3) if which == "off_grid" else fl.times4(s)
        x.tofile(tmp_path / "x.f32")
        r = subprocess.run([mirror_exe, str(tmp_path / "x.f32")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (which, c, r.stdout[-1500:], r.stderr[-1500:])
        n_frames, n_diag = [int(v) for v in r.stdout.split()[-2:]]
        assert n_frames >= 2 and n_diag > 10, r.stdout
