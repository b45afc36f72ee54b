"""GPU tests of complex IQ input (ABI 608, include/m17hip.h: m17hip_upload_iq and friends): the FM discriminator kernel writes the float input slab, and
from there on the stream is a float stream.  Every comparison is exact: the discriminated floats (m17hip_download_f32) as uint32 words against the HOST
form of the same arithmetic (tests/cxx/iq_oracle.cpp: detail/core.h under the host compiler) — NaN-ness where that is a NaN — and records, m17_diag and
the diagnostic log byte for byte against the float oracle (tests/cxx/f32_oracle.cpp) stepped on the host form's floats.  What the host form itself is
worth is asserted without a GPU in tests/test_iq_input.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
THREADS = 16
INV = m17hip.FLAG_INVERT
INT_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock")
FMTS = {"i16": iq.IQ_I16, "f32": iq.IQ_F32}
GAINS = (1.0, 5.0 / 3.0)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_words(got, exp, what):
    """Equal words; where the host form gives a NaN, a NaN (payload unspecified)."""
    nan = np.isnan(exp)
    assert np.isnan(got[nan]).all(), (what, "NaN expected")
    bad = np.argwhere((_u32(got) != _u32(exp)) & ~nan)
    assert bad.size == 0, (what, bad[:8].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _dev(a):
    """The array on the device, COMPLETE when this returns (the context's streams do not wait for torch's)."""
    import torch
    t = torch.from_numpy(np.array(a)).cuda()   # (a writable copy: the fixtures are read-only)
    torch.cuda.synchronize()
    return t


def _raw(ctx, name, ptr, Cn, T, pitch, fmt, gain=1.0):
    return getattr(ctx.lib, name)(ctx.h, C.c_void_p(ptr), C.c_int(fmt), C.c_float(gain), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(pitch))


def _sample_bytes(fmt):
    return 4 if fmt == iq.IQ_I16 else 8


# ---- 1: one hop ----------------------------------------------------------------------------------------------------------------------------------
# a lane takes 4 samples, a wave 256, a workgroup 1024: those edges +- 1 (and two sizes of several workgroups)
HOP_C, HOP_TS = (1, 3, 65), (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 4097)
HOP_PITCH = max(HOP_TS) + 2   # odd: row c begins 16-byte aligned only for even c (float IQ) / c = 0 mod 4 (int16 IQ) — both paths of the kernel in every launch
BAD_ROW = 1                   # the float row that holds infinities and NaNs


def _spice(z, rng):
    """Components up to +-1e9, denormals of magnitude 1e-40 and +-0 sprinkled over every row of complex64 z."""
    v = z.view(np.float32).reshape(z.shape[0], -1)
    n = v.shape[1]
    for row in v:
        k = max(1, n // 11)
        row[rng.integers(0, n, k)] = (10.0 ** rng.uniform(0, 9, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)
        row[rng.integers(0, n, k)] = np.float32(1e-40) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), k)
        row[rng.integers(0, n, k)] = rng.choice(np.array([-0.0, 0.0], dtype=np.float32), k)
        row[2 * rng.integers(1, n // 2, 3) + 1] = 0.0   # (and whole zero samples: a zero product)
    return z


@pytest.fixture(scope="module")
def hop_case():
    rng = np.random.default_rng(608)
    Cn, P = max(HOP_C), HOP_PITCH
    xi = rng.integers(-32768, 32768, size=(Cn, P, 2)).astype(np.int16)
    xi[:, 5] = (-32768, 32767)
    xi[:, 9] = 0
    xf = (12000.0 * (rng.standard_normal((Cn, P)) + 1j * rng.standard_normal((Cn, P)))).astype(np.complex64)
    xf[:, 8:10] = 0
    xf = _spice(xf, rng)
    v = xf[BAD_ROW].view(np.float32)
    for k, val in zip(rng.choice(np.arange(40, 2 * max(HOP_TS), 97), 9, replace=False), [np.inf, -np.inf, np.nan] * 3):
        v[k] = val
    v[6] = np.inf   # (early enough for the short slabs: samples 3 and 4 are poisoned)
    assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(xf.view(np.float32)) > 1e8).any()
    data = {iq.IQ_I16: xi, iq.IQ_F32: xf}
    # a fresh feed each time: y[t] depends on x[0 .. t] alone, the expectation of a shorter slab is a prefix of the longest one's
    exp = {(f, g): iq.discriminate_rows(d[:, : max(HOP_TS)], g)[0] for f, d in data.items() for g in GAINS}
    assert np.isnan(exp[iq.IQ_F32, 1.0][BAD_ROW]).any() and np.isfinite(np.delete(exp[iq.IQ_F32, 1.0], BAD_ROW, axis=0)).all()
    for a in list(data.values()) + list(exp.values()):
        a.setflags(write=False)
    return data, exp


@pytest.mark.parametrize("Cn", HOP_C)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_discriminator_one_hop(hop_case, fmt, Cn):
    """Host and device sources, pitch > samples with aligned and unaligned rows, both gains, every lane / wave / workgroup edge: the host form's words.
    The float rows hold values up to 1e9, denormals and zeroes; one of them infinities and NaNs, which stay in it."""
    data, exp = hop_case
    f = FMTS[fmt]
    host = data[f]
    dev = _dev(host)
    ctx = m17hip.Context(max(HOP_C), max(HOP_TS))
    try:
        for T in HOP_TS:
            for gain in GAINS:
                for src in ("host", "device"):
                    ctx.reset()   # (a fresh feed: the carry is zero)
                    name, ptr = ("m17hip_upload_iq", host.ctypes.data) if src == "host" else ("m17hip_upload_iq_device", dev.data_ptr())
                    assert _raw(ctx, name, ptr, Cn, T, HOP_PITCH, f, gain) == 0
                    ctx.C, ctx.T = Cn, T
                    assert ctx.input_format()[0] == m17hip.FORMAT_F32
                    _assert_words(ctx.download_f32(), exp[f, gain][:Cn, :T], (fmt, Cn, T, gain, src))
    finally:
        ctx.close()


# ---- 2: the feed ---------------------------------------------------------------------------------------------------------------------------------
FEED_C, FEED_T = 5, 5000
FEED_CUTS = np.cumsum([0, 1, 2, 255, 1024]).tolist() + [FEED_T]


@pytest.fixture(scope="module")
def feed_case():
    """Integer-valued IQ in both layouts (the same samples: the format may change from block to block) and its one-block result."""
    rng = np.random.default_rng(6081)
    s = rng.integers(-21504, 21505, size=(FEED_C, FEED_T)).astype(np.int16)
    xi = iq.fm_modulate(s, sigma=400.0, cfo=0.01, fmt=iq.IQ_I16, seed=3)
    xf = (xi[..., 0].astype(np.float32) + 1j * xi[..., 1].astype(np.float32)).astype(np.complex64)
    whole = iq.discriminate_rows(xi, 1.25)[0]
    assert np.array_equal(_u32(whole), _u32(iq.discriminate_rows(xf, 1.25)[0]))
    for a in (xi, xf, whole):
        a.setflags(write=False)
    return {iq.IQ_I16: xi, iq.IQ_F32: xf}, whole


@pytest.mark.parametrize("plan", ["i16", "f32", "switching"])
def test_blocks_continue_one_another_in_call_order(feed_case, plan):
    """Several in-place uploads on one context, no run in between: the concatenated downloads are the one-block result."""
    data, whole = feed_case
    dev = {f: _dev(a) for f, a in data.items()}
    ctx = m17hip.Context(FEED_C, FEED_T)
    try:
        for src in ("host", "device"):
            ctx.reset()
            parts = []
            for k, (a, b) in enumerate(zip(FEED_CUTS[:-1], FEED_CUTS[1:])):
                f = FMTS[plan] if plan != "switching" else (iq.IQ_I16, iq.IQ_F32)[(k + (src == "device")) & 1]
                if src == "host":
                    ctx.upload_iq(data[f][:, a:b], gain=1.25)
                else:
                    ctx.upload_iq_device(dev[f].data_ptr() + a * _sample_bytes(f), FEED_C, b - a, pitch=FEED_T, iq_format=f, gain=1.25)
                parts.append(ctx.download_f32())
            _assert_words(np.concatenate(parts, axis=1), whole, (plan, src))
    finally:
        ctx.close()


@pytest.mark.parametrize("source", ["pinned", "device"])
def test_the_carry_crosses_between_the_main_and_the_copy_stream(feed_case, source):
    """In-place blocks run on the main stream, staged ones on the copy stream: each finds the carry the block before it left, whichever stream that ran
    on.  A staged block's floats are read back once a run has taken its slab; a staged block nobody runs still passes its carry on."""
    import torch
    data, whole = feed_case
    f = iq.IQ_F32 if source == "device" else iq.IQ_I16
    dev = _dev(data[f])
    pin = torch.from_numpy(np.array(data[f])).pin_memory()
    sb = _sample_bytes(f)
    ctx = m17hip.Context(FEED_C, FEED_T)
    try:
        ctx.reset()

        def stage(a, b):
            if source == "device":
                ctx.upload_iq_device_async(dev.data_ptr() + a * sb, FEED_C, b - a, pitch=FEED_T, iq_format=f, gain=1.25)
            else:
                ctx.upload_iq_async(pin.data_ptr() + a * sb, FEED_C, b - a, pitch=FEED_T, iq_format=f, gain=1.25)

        def in_place(a, b):
            ctx.upload_iq_device(dev.data_ptr() + a * sb, FEED_C, b - a, pitch=FEED_T, iq_format=f, gain=1.25)

        cuts = [0, 1, 3, 258, 1282, 2306, 3000, FEED_T]
        how = ["in_place", "in_place", "staged_run", "in_place", "staged_only", "in_place", "staged_run"]
        for (a, b), h in zip(zip(cuts[:-1], cuts[1:]), how):
            if h == "in_place":
                in_place(a, b)
            else:
                stage(a, b)
                if h == "staged_only":
                    continue
                ctx.run(channels=FEED_C, samples=b - a)
            _assert_words(ctx.download_f32(), whole[:, a:b], (source, h, a, b))
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: the full chain ---------------------------------------------------------------------------------------------------------------------------
CH_T = 30720   # 160 ticks of 192
CH_KINDS, CH_CHANNELS = (0, 1, 2, 4), ((300.0, 0.0), (1500.0, 0.02))
CH_C = len(CH_KINDS) * len(CH_CHANNELS)
LOG_CAP = CH_T // 384 + 2


class Expect:
    """The float oracle over whole streams y[C][T] (channel c under invert[c], from sample origin[c] on): records and log entries of the run that
    covers samples [b0, b1) of the context's stream, and m17_diag at the end of the stream."""

    def __init__(self, y, invert=None, origin=None):
        self.C, self.T = y.shape
        self.origin = np.zeros(self.C, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
        self.recs, self.logs, self.diags = [None] * self.C, [None] * self.C, np.zeros(self.C, dtype=ol.DIAG)
        inv = np.zeros(self.C, dtype=np.uint8) if invert is None else np.broadcast_to(np.asarray(invert, dtype=np.uint8), (self.C,))
        for a in np.unique(self.origin):
            chs = np.flatnonzero(self.origin == a)
            r, n, d, lg, ln = fl.demod_batch(np.ascontiguousarray(y[chs, a:]), invert=inv[chs], threads=THREADS, logs=True)
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
            rows.append(r[(r["sample_pos"] >= max(lo, 0)) & (r["sample_pos"] < hi)].copy())
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
        glog = ctx.diag_log(Cn, capacity=LOG_CAP)
        for c in range(Cn):
            assert glog[c].tobytes() == logs[c].tobytes(), (what, "diagnostic log", c, glog[c].size, logs[c].size)
    if diags is not None:
        d = ctx.diag(Cn)
        for fld in INT_FIELDS:
            assert np.array_equal(d[fld], diags[fld]), (what, fld, np.flatnonzero(d[fld] != diags[fld])[:16].tolist())
        for fld in FLOAT_FIELDS:
            assert np.array_equal(d[fld], diags[fld], equal_nan=True), (what, fld)


def _ctx(Cn, T, log=True):
    ctx = m17hip.Context(Cn, T)
    if log:
        ctx.tune(9, LOG_CAP)
    return ctx


@pytest.fixture(scope="module")
def chain_case():
    """Eight transmitters — BERT, stream and both packet kinds, each over a quiet and a noisy, off-frequency channel — as baseband, as IQ in both
    layouts, and the host form's floats with the float oracle's verdict on them."""
    s = np.zeros((CH_C, CH_T), dtype=np.int16)
    x = {iq.IQ_I16: np.zeros((CH_C, CH_T, 2), dtype=np.int16), iq.IQ_F32: np.zeros((CH_C, CH_T), dtype=np.complex64)}
    for c in range(CH_C):
        kind, (sigma, cfo) = CH_KINDS[c % 4], CH_CHANNELS[c // 4]
        s[c] = ol.generate(ol.gen_params(seed=1, kind=kind, lead_in=9600, n_frames=6, tail=4800, total=CH_T))[:CH_T]
        for f in x:
            x[f][c] = iq.fm_modulate(s[c], sigma=sigma, cfo=cfo, fmt=f, seed=1)
    y = {f: iq.discriminate_rows(x[f], 1.0)[0] for f in x}
    exp = {f: Expect(y[f]) for f in x}
    for f in x:
        assert all(r.size >= 6 for r in exp[f].recs), "every channel yields frames"
        x[f].setflags(write=False)
        y[f].setflags(write=False)
    return s, x, y, exp


@pytest.mark.parametrize("src", ["host", "tensor"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_full_chain_in_one_run(chain_case, fmt, src):
    _, x, y, exp = chain_case
    f = FMTS[fmt]
    ctx = _ctx(CH_C, CH_T)
    try:
        ctx.reset()
        if src == "host":
            ctx.upload_iq(x[f])
        else:
            ctx.upload_iq(_dev(x[f]))   # (a complex64 [C][T] or an int16 [C][T][2] tensor on the device: read where it lies)
        _assert_words(ctx.download_f32(), y[f], (fmt, src))
        ctx.run()
        rows, logs = exp[f].run(0, CH_T)
        _check(ctx, rows, logs, f"{fmt} {src}", diags=exp[f].diags)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_full_chain_pipelined_in_ragged_segments(chain_case, fmt, order):
    """A live feed: m17hip_upload_iq_device_async of segment k + 1, m17hip_demod_front, run — the discriminator of the next segment on the copy stream
    beside the state-machine half of the current run; segments of ragged multiples of 192."""
    _, x, _, exp = chain_case
    f = FMTS[fmt]
    b = [0, 192, 192 * 27, 192 * 28, 192 * 75, 192 * 131, CH_T]
    lens = [b1 - b0 for b0, b1 in zip(b[:-1], b[1:])]
    dev = _dev(x[f])
    sb = _sample_bytes(f)
    ctx = _ctx(CH_C, max(lens), log=False)
    try:
        ctx.reset()

        def stage(k):
            ctx.upload_iq_device_async(dev.data_ptr() + b[k] * sb, CH_C, lens[k], pitch=CH_T, iq_format=f)

        stage(0)
        ctx.run(channels=CH_C, samples=lens[0])
        for k in range(len(lens)):
            more = k + 1 < len(lens)
            if more:
                stage(k + 1)
                ctx.front(channels=CH_C, samples=lens[k + 1])
                if order == "run_then_fetch":
                    ctx.run(channels=CH_C, samples=lens[k + 1])
                    ctx.frames_select(1)
            got = ctx.frames().copy()
            ctx.frames_select(0)
            rows, _ = exp[f].run(b[k], b[k + 1])
            _check(ctx, rows, None, f"pipelined {fmt} {order}, segment {k}", diags=None if more else exp[f].diags, got=got)
            if more and order != "run_then_fetch":
                ctx.run(channels=CH_C, samples=lens[k + 1])
        ctx.upload_wait()
        assert ctx.input_format()[0] == m17hip.FORMAT_F32
    finally:
        ctx.close()


def test_full_chain_mixed_polarity_with_conjugated_input(chain_case):
    """The inverted channels receive the conjugate (the spectrum flipped): its discriminated floats are the negation, which the polarity table undoes."""
    _, x, y, exp = chain_case
    f = iq.IQ_F32
    pol = np.array([0, 1, 1, 0, 1, 0, 0, 1], dtype=np.uint8)
    xm = np.where(pol[:, None] == 1, np.conj(x[f]), x[f])
    ym = iq.discriminate_rows(xm, 1.0)[0]
    em = Expect(ym, invert=pol)
    for c in range(CH_C):   # (the premise: under its polarity every channel carries what the plain one carries)
        assert em.recs[c]["payload"].tobytes() == exp[f].recs[c]["payload"].tobytes(), c
    rows, logs = em.run(0, CH_T)
    ctx = _ctx(CH_C, CH_T)
    try:
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_iq(xm)
        ctx.run()
        _check(ctx, rows, logs, "mixed table", diags=em.diags)
        ctx.set_channel_polarity(pol ^ 1)   # (every entry changes: all channels start over) and the flag turns them back
        ctx.reset()
        ctx.upload_iq(xm)
        ctx.run(flags=INV)
        _check(ctx, rows, logs, "mixed table, flagged", diags=em.diags)
    finally:
        ctx.close()


def test_reset_channels_starts_the_listed_feeds_over(chain_case):
    """Three runs of 10 240 samples; three channels start over in front of the second upload (on the tick grid): their IQ feed begins from a zero carry
    there — the first float is +0 — and their demodulators are fresh; the others continue."""
    _, x, y, _ = chain_case
    f = iq.IQ_I16
    T, n_runs = 192 * 53, 3
    total = T * n_runs
    again = np.array([1, 2, 6])
    origin = np.zeros(CH_C, dtype=np.int64)
    origin[again] = T
    ye = np.array(y[f][:, :total])
    for c in again:
        ye[c, T:] = iq.discriminate(x[f][c, T:total], 1.0, None)[0]
        assert ye[c, T] == 0 and y[f][c, T] != 0
    exp = Expect(ye, origin=origin)
    first = Expect(np.ascontiguousarray(ye[again, :T]))
    ctx = _ctx(CH_C, T)
    try:
        ctx.reset()
        for r in range(n_runs):
            if r == 1:
                ctx.reset_channels(again)
            ctx.upload_iq(x[f][:, r * T:(r + 1) * T])
            _assert_words(ctx.download_f32(), ye[:, r * T:(r + 1) * T], f"floats of run {r}")
            ctx.run()
            rows, logs = exp.run(r * T, (r + 1) * T)
            if r == 0:   # (before they start over, the channels concerned are channels like any other: from the stream's start)
                for i, c in enumerate(again):
                    rows[c], logs[c] = first.recs[i].copy(), first.logs[i]
                    rows[c]["channel"] = c
            _check(ctx, rows, logs, f"run {r}", diags=exp.diags if r + 1 == n_runs else None)
        assert sum(r.size for r in exp.recs) > CH_C
    finally:
        ctx.close()


# ---- 4: state rules ------------------------------------------------------------------------------------------------------------------------------
def test_format_rule_memory_and_timing(chain_case):
    s, x, y, _ = chain_case
    Cn, T = 4, 9600
    si = np.ascontiguousarray(s[:Cn, :T])
    xi, xf = np.ascontiguousarray(x[iq.IQ_I16][:Cn, :T]), np.ascontiguousarray(x[iq.IQ_F32][:Cn, :T])
    dev = _dev(xf)
    ctx = m17hip.Context(Cn + 2, T)
    try:
        # a context that only ever sees int16 holds nothing for IQ and nothing for floats
        assert ctx.iq_bytes() == 0 and ctx.input_format() == (0, 0)
        ctx.upload(si)
        ctx.run()
        assert ctx.iq_bytes() == 0 and ctx.input_format() == (m17hip.FORMAT_I16, 0)
        # an IQ upload on an int16 stream: refused, nothing changed
        for name, ptr in (("m17hip_upload_iq", xf.ctypes.data), ("m17hip_upload_iq_device", dev.data_ptr()), ("m17hip_upload_iq_device_async", dev.data_ptr()),
                          ("m17hip_upload_iq_async", xf.ctypes.data)):
            assert _raw(ctx, name, ptr, Cn, T, T, iq.IQ_F32) == ESTATE, name
        assert ctx.iq_bytes() == 0 and ctx.input_format() == (m17hip.FORMAT_I16, 0)
        assert ctx.download().tobytes() == si.tobytes()
        ctx.reset()   # frees the choice
        ctx.timing(True)
        ctx.upload_iq_device(dev.data_ptr(), Cn, T, iq_format=iq.IQ_F32)
        assert ctx.iq_bytes() == (Cn + 2) * 8, "device forms hold the carry alone"
        fmt, fbytes = ctx.input_format()
        assert fmt == m17hip.FORMAT_F32 and fbytes >= Cn * T * 4
        _assert_words(ctx.download_f32(), y[iq.IQ_F32][:Cn, :T], "device")
        ctx.reset()
        ctx.upload_iq(xi)
        assert ctx.iq_bytes() == (Cn + 2) * 8 + Cn * T * 4, "and the host forms the raw block"
        ctx.reset()
        ctx.upload_iq(xf)   # (a larger block: the buffer grows)
        assert ctx.iq_bytes() == (Cn + 2) * 8 + Cn * T * 8
        _assert_words(ctx.download_f32(), y[iq.IQ_F32][:Cn, :T], "host")
        ms, launches = ctx.timing_get("discriminate")
        assert launches == 3 and ms > 0
        ctx.timing(False)
        ctx.run()
        # the stream the discriminator made is a float stream: int16 input and synthesis are refused
        out = np.zeros((Cn, T), dtype=np.int16)
        assert ctx.lib.m17hip_upload_i16(ctx.h, ol._p(si), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(T)) == ESTATE
        assert ctx.lib.m17hip_download_i16(ctx.h, ol._p(out), C.c_uint32(Cn), C.c_uint32(T), C.c_size_t(T)) == ESTATE
        p = ol.gen_params(seed=3, kind=1, n_frames=2, total=T)
        assert ctx.lib.m17hip_synth_i16(ctx.h, C.byref(p), C.c_uint32(Cn), C.c_uint32(T), C.c_uint32(0)) == ESTATE
        ctx.upload(fl.on_grid(si))   # (floats are welcome: it is a float stream)
        ctx.run()
    finally:
        ctx.close()


def test_argument_refusals_and_the_queued_front_end(chain_case):
    import torch
    _, x, _, _ = chain_case
    Cn, T = 4, 1920
    xf = np.ascontiguousarray(x[iq.IQ_F32][:Cn, :T])
    dev, pin = _dev(xf), torch.from_numpy(xf.copy()).pin_memory()
    ctx = m17hip.Context(Cn, T)
    try:
        for name, ptr in (("m17hip_upload_iq", xf.ctypes.data), ("m17hip_upload_iq_async", pin.data_ptr()), ("m17hip_upload_iq_device", dev.data_ptr()),
                          ("m17hip_upload_iq_device_async", dev.data_ptr())):
            assert _raw(ctx, name, None, Cn, T, T, iq.IQ_F32) == EINVAL, name
            assert _raw(ctx, name, ptr, 0, T, T, iq.IQ_F32) == EINVAL, name
            assert _raw(ctx, name, ptr, Cn, 0, T, iq.IQ_F32) == EINVAL, name
            assert _raw(ctx, name, ptr, Cn + 1, T, T, iq.IQ_F32) == EINVAL, name
            assert _raw(ctx, name, ptr, Cn, T + 1, T + 1, iq.IQ_F32) == EINVAL, name
            assert _raw(ctx, name, ptr, Cn, T, T - 1, iq.IQ_F32) == EINVAL, name
            for bad_fmt in (0, 3, -1):
                assert _raw(ctx, name, ptr, Cn, T, T, bad_fmt) == EINVAL, name
            for bad_gain in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
                assert _raw(ctx, name, ptr, Cn, T, T, iq.IQ_F32, bad_gain) == EINVAL, (name, bad_gain)
        assert ctx.lib.m17hip_iq_bytes(ctx.h, None) == EINVAL
        assert ctx.iq_bytes() == 0 and ctx.input_format() == (0, 0), "a refused call changes nothing"
        # while a front end queued by m17hip_demod_front waits for its run, the slabs are its own
        ctx.upload_iq_device_async(dev.data_ptr(), Cn, T)
        ctx.run(channels=Cn, samples=T)
        ctx.upload_iq_device_async(dev.data_ptr(), Cn, T)
        ctx.front(channels=Cn, samples=T)
        for name, ptr in (("m17hip_upload_iq", xf.ctypes.data), ("m17hip_upload_iq_async", pin.data_ptr()), ("m17hip_upload_iq_device", dev.data_ptr()),
                          ("m17hip_upload_iq_device_async", dev.data_ptr())):
            assert _raw(ctx, name, ptr, Cn, T, T, iq.IQ_F32) == ESTATE, name
        ctx.run(channels=Cn, samples=T)
        ctx.upload_wait()
        ctx.frames()
    finally:
        ctx.close()


# ---- 5: the example ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
def test_example_discriminates_on_the_device(chain_case, fmt):
    """examples/m17-demod-gpu --iq-*: M17Demodulator<float>::iq buffers the IQ and uploads it block by block (m17hip_upload_iq, the feed carried on the
    device); its frame callbacks are the float oracle's on the host form's floats, in order."""
    _, x, y, _ = chain_case
    f = FMTS[fmt]
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    c = 1   # (a stream transmission over the quiet channel)
    out = subprocess.run([exe, "--iq-" + fmt], input=np.ascontiguousarray(x[f][c]).tobytes(), capture_output=True, check=True, timeout=120).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    recs, _ = fl.demod(y[f][c])
    exp = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == exp and len(exp) >= 6
