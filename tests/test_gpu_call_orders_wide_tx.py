"""GPU tests of the WIDEBAND SIGNAL GENERATOR (ABI 617: m17hip_synth_wide_config, m17hip_synth_wide_channels, m17hip_synth_wide, m17hip_synth_wide_device;
synth_wide in csrc/m17hip.hip) beside runs and receivers in flight.  tests/test_gpu_wide_tx.py compares its bytes with the host form's on single blocks
of an idle device; the generator reads c->now()'s slab on the main stream, though, and a context may at that moment have a demodulation run in flight on
that slab, a staged input waiting in the other one, tuning key 16 on (the in-place producers write the staging slab) or a slab swap queued by
m17hip_demod_run — and its carries (A2, two copies of the last sample) and its turn-taking device table cross all of these.

B1 - B4, a TX context whose own stream is busy: the regime is tests/test_gpu_call_orders.py's, imported as it stands — 4096 channels, its Stream (x, the
oracle's records; the fixtures voice and consumers), run 0 of 96 000 samples whose 7.4 - 8.6 ms on the main stream is that module's measured premise,
asserted with the parents' _in_flight.  The generator has 2 sources at 5 / 1, int16 output, noise sigma 50, M17's deviation word; 16 of the 4096 channels
are audible (8 per source, 12.5 kHz apart inside +-100 kHz, amplitude 4000: 8 x 4000 + 8 x 50 <= 32 767, no sample clips); the silent ones are left out
of the device lists, and the host form (wide_tx_lib.Mux with channels = 4096, through SparseMux below) moves their carries without modulating them: one
block of 96 000 samples is 0.4 s of host form.  Bytes are compared with tests/test_gpu_wide_tx.py's _same.

B5, TX feeds RX through two device buffers block after block: the RX context is the parent's context() of tests/test_gpu_call_orders_resample.py
(128 / 3) or of tests/test_gpu_call_orders_wide2.py (50 / 1) with 4096 channels; the TX context has 8 channels of oracle_lib basebands made as the
parents' sources() makes them, at the parents' offsets and noise.  The premise there is the parents' (D from their fixture tuner_s, _made_under_the_tuner).
"""
import ctypes as C
import time

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import test_gpu_call_orders as po
import test_gpu_call_orders_resample as pr
import test_gpu_call_orders_wide2 as p2
import test_gpu_wide_tx as gtw
import test_resample_input as cpu
import wide_lib as wl
import wide_tx_lib as wt
from test_gpu_call_orders import CN, DIAG_EXACT, DIAG_FLOAT, DIAG_STREAM, T0, T1, _check_bert, _check_diag, _check_packets, _check_records, _frames_once, consumers, voice  # noqa: F401
from test_gpu_call_orders_formats import Expect, _check_words, _in_flight
from test_gpu_call_orders_resample import case, first_staging_of_the_process, run0_floats  # noqa: F401
from test_gpu_call_orders_resample import tuner_s as tuner_resample_s  # noqa: F401
from test_gpu_call_orders_wide2 import ALL, REP, TB, _made_under_the_tuner, cases, rep, rep_rows  # noqa: F401
from test_gpu_call_orders_wide2 import tuner_s as tuner_wide2_s  # noqa: F401
from test_gpu_wide_tx import ESTATE, PAD, _same, _sentinel, _synth

pytestmark = pytest.mark.gpu

# ---- B1 - B4: the generator of a TX context whose own stream is busy ----------------------------------------------------------------------------------------
GS, GP, GQ, GFMT = 2, 5, 1, wt.IQ_I16
GSIGMA, GSEED, GA = 50.0, 617, 4000.0
PER = 8                                             # audible channels per source
AUDIBLE = np.arange(GS * PER) * 256 + 3             # 16 of the 4096 channels, spread over the context
LATE = int(AUDIBLE[5]) + 1                          # silent in block 1, audible in block 2 of B4
assert PER * GA + 8.0 * GSIGMA <= 32767.0 and AUDIBLE.max() < CN and LATE not in AUDIBLE
NAMES = {"device": "m17hip_synth_wide_device", "host": "m17hip_synth_wide"}


def table(late=False):
    """(source, fcw, phase0, amplitude) for all 4096 channels: channel AUDIBLE[i] on source i % 2 at 12.5 kHz x (i // 2 - 4), everybody else silent.
    late: LATE transmits as well, at +75 kHz on source 1, and AUDIBLE[2] has moved to -87.5 kHz."""
    src, fcw = np.zeros(CN, dtype=np.uint32), np.zeros(CN, dtype=np.int64)
    ph, amp = np.zeros(CN, dtype=np.int64), np.zeros(CN, dtype=np.float32)
    for i, c in enumerate(AUDIBLE):
        src[c], fcw[c], ph[c], amp[c] = i % GS, m17hip.wide_fcw(12500.0 * (i // GS - 4), GP / GQ), (i * 0x9E3779B1) & 0xFFFFFFFF, GA
    if late:
        src[LATE], fcw[LATE], ph[LATE], amp[LATE] = 1, m17hip.wide_fcw(75000.0, GP / GQ), 77, GA / 2
        fcw[AUDIBLE[2]] = m17hip.wide_fcw(-87500.0, GP / GQ)
    assert np.abs(fcw.astype(np.float64)).max() < 100e3 / (48000.0 * GP / GQ) * 2.0 ** 32
    return src, fcw, ph, amp


class SparseMux(wt.Mux):
    """wide_tx_lib.Mux for a table whose channels are nearly all silent.  A term of amplitude 0 leaves the chain's words as they are (include/m17hip.h), so
    the silent channels' part in a block is their carries alone: A2 += b[-1] + 2 (b[0] + ... + b[n-2]) + b[n-1] modulo 2^64 and last = b[n-1] — the sum the
    definition's A2[n] is, which Mux itself computes sample by sample (check_carries compares the two on the host).  The audible channels go through
    Mux.floats as they stand, in ascending channel order."""

    def floats(self, x, wrong=0):
        x = np.ascontiguousarray(x, dtype=np.int16)
        Cn, n = x.shape
        aud = np.flatnonzero(self.table["amplitude"][:Cn] > 0)
        inner = wt.Mux(self.S, self.P, self.Q, self.K, self.fmt, self.sigma, self.seed, 0, channels=aud.size)
        inner.table[:] = self.table[aud]
        inner.a2, inner.last, inner.count = self.a2[aud].copy(), self.last[aud].copy(), self.count
        out = inner.floats(x[aud], wrong)
        total = self.last[:Cn].astype(np.int64) + 2 * x[:, :-1].sum(axis=1, dtype=np.int64) + x[:, -1].astype(np.int64)
        self.a2[:Cn] = (self.a2[:Cn].astype(object) + total.astype(object)) % (1 << 64)
        self.last[:Cn] = x[:, -1]
        assert np.array_equal(self.a2[aud], inner.a2) and np.array_equal(self.last[aud], inner.last)
        self.count = inner.count
        return out


def check_carries(x):
    """The closed form of a silent channel's carries against wide_tx_lib.theta's, on three rows and from carries that are not zero."""
    for c in (0, LATE, CN - 1):
        m = SparseMux(GS, GP, GQ, wt.k_stated(GP), GFMT, 0.0, 0, 0, channels=CN)
        m.a2[c], m.last[c] = 0xFFFFFFFFFFFF0000, -12345
        _, a2, last = wt.theta(x[c], GP, GQ, m.K, a2=int(m.a2[c]), last=int(m.last[c]))
        m.floats(x)
        assert (int(m.a2[c]), int(m.last[c])) == (a2, last), c


def host_form(sigma=GSIGMA, seed=GSEED, first=0, late=False):
    m = SparseMux(GS, GP, GQ, wt.k_stated(GP), GFMT, sigma, seed, first, channels=CN)
    m.channels(*table(late))
    return m


def tx_context(maxT=T0, keys=(), sigma=GSIGMA, seed=GSEED, first=0):
    ctx = m17hip.Context(CN, maxT)
    try:
        for k in keys:
            ctx.tune(k, CN if k == 7 else 1)
        ctx.synth_wide_config(GS, GP, GQ, GFMT, None, sigma, seed, first)
        ctx.synth_wide_channels(*table())
    except Exception:
        ctx.close()
        raise
    return ctx


def _out(n):
    """A device tensor for one block of n baseband samples, made (and the device synchronised) BEFORE the run a case wants in flight is queued."""
    return _sentinel(GS, n // GQ * GP + PAD, GFMT)


def _generate(ctx, form, n, what, exp, t=None):
    """One block of the generator over the `CN` x `n` input the current slab holds, by the host form of the call or into the device tensor t (_out),
    compared with the host form's bytes."""
    W = n // GQ * GP
    if form == "host":
        got = ctx.synth_wide(samples=n, channels=CN)
    else:
        ctx.synth_wide(samples=n, out=t, channels=CN)
        a = t.cpu().numpy()
        assert (a[:, W:] == 77).all() and a.shape[1] == W + PAD, "nothing behind a row's W samples is written"
        got = np.ascontiguousarray(a[:, :W])
    _same(got, exp, what)
    assert int(got.max()) < 32767 and int(got.min()) > -32768, "no sample clips"


def _download(ctx, n):
    """(code, rows) of m17hip_download_i16 for CN x n samples: what the generator would modulate at this moment."""
    out = np.full((CN, n), 77, dtype=np.int16)
    code = ctx.lib.m17hip_download_i16(ctx.h, m17hip._ptr(out), C.c_uint32(CN), C.c_uint32(n), C.c_size_t(n))
    return code, out


def _refused(ctx, n, what):
    """Where m17hip_download_i16 is M17HIP_ESTATE the generator is as well, by both forms, and nothing is written."""
    assert _download(ctx, n)[0] == ESTATE, what
    W = n // GQ * GP
    dev, host = _sentinel(GS, W, GFMT), np.full((GS, W, 2), 77, dtype=np.int16)
    assert _synth(ctx, NAMES["device"], dev.data_ptr(), CN, n, W) == ESTATE and _synth(ctx, NAMES["host"], host.ctypes.data, CN, n, W) == ESTATE, what
    import torch
    torch.cuda.synchronize()
    assert (host == 77).all() and dev.cpu().numpy().tobytes() == host.tobytes(), what


def _run_0(ctx, s, where="device"):
    """Run 0's input in place, the run queued, and the premise: it is in flight."""
    if where == "device":
        ctx.upload_device(s.dev.data_ptr(), CN, T0, pitch=T0 + T1)
    else:
        ctx.upload(s.x0)
    ctx.run()
    _in_flight(ctx)


def _run_0_is(ctx, s, keys=()):
    """Run 0's records, m17_diag and consumers are the oracle's: the generator moved nothing."""
    assert ctx.frames_count() == s.rec0.size
    _check_records(_frames_once(ctx), s.rec0)
    _check_diag(ctx.diag(CN), s.diag0, DIAG_EXACT + DIAG_FLOAT)
    if 6 in keys:
        _check_bert(ctx.bert_stats(CN), s.bert0)
    if 7 in keys:
        _check_packets(ctx.packets(capacity=4 * CN), s.pk0)


@pytest.fixture(scope="module")
def blocks(voice):
    """The host form's bytes of the blocks every case begins with, computed once: block 1 over run 0's input, and the feed's state behind it."""
    check_carries(voice.x0[:, :1920])
    m = host_form()
    first = m.block(voice.x0)
    first.setflags(write=False)
    return {"first": first, "behind": m}


def _behind(blocks):
    import copy
    return copy.deepcopy(blocks["behind"])


# ---- B1 -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,stream", [("device", "voice"), ("host", "voice"), ("device", "consumers")])
def test_generator_at_once_behind_a_run_in_flight(request, blocks, form, stream):
    """Run 0's input uploaded in place, the run queued (in flight: asserted), and the generator called at once: it reads the slab beside K1 to K5.  Its
    bytes are the host form's; run 0's records, m17_diag and — on the parent's consumer stream, with tuning keys 6 and 7 — the PRBS9 counts and packets
    are the oracle's byte for byte."""
    s = request.getfixturevalue(stream)
    keys = (6, 7) if stream == "consumers" else ()
    exp = blocks["first"] if stream == "voice" else host_form().block(s.x0)
    t = _out(T0) if form == "device" else None
    ctx = tx_context(keys=keys)
    try:
        _run_0(ctx, s)
        _generate(ctx, form, T0, (form, stream), exp, t)
        _run_0_is(ctx, s, keys)
    finally:
        ctx.close()


# ---- B2 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_generator_beside_a_staged_input_that_has_not_run(voice, blocks):
    """Behind B1's block: the next 24 000 samples staged from pinned memory, no run.  The generator modulates what m17hip_download_i16 returns at that
    moment — the CURRENT slab, run 0's input again — with its carries continued; then m17hip_demod_run swaps the slabs (in flight: asserted) and the
    generator, at once, modulates the new one."""
    s = voice
    m = _behind(blocks)
    again = m.block(s.x0)
    assert all((again[k, :5] != blocks["first"][k, :5]).any() for k in range(GS)), "a fresh feed's first samples are others"
    zero = _behind(blocks)
    zero.a2[:], zero.last[:] = 0, 0
    assert all((again[k, :5] != zero.block(s.x0)[k, :5]).any() for k in range(GS)), "the carries decide the block's first samples"
    nxt = m.block(s.x1["full"])
    t1, t2, t3 = _out(T0), _out(T0), _out(T1)
    ctx = tx_context()
    try:
        _run_0(ctx, s)
        _generate(ctx, "device", T0, "block 1", blocks["first"], t1)
        ctx.upload_async(s.pin1["full"].data_ptr(), CN, T1)
        code, rows = _download(ctx, T0)
        assert code == 0 and np.array_equal(rows, s.x0), "the current slab is run 0's"
        _generate(ctx, "device", T0, "the current slab beside a staged input", again, t2)
        ctx.run(channels=CN, samples=T1)
        _in_flight(ctx, "run 1")
        _generate(ctx, "device", T1, "the new slab behind the swap", nxt, t3)
        assert _download(ctx, T1)[1].tobytes() == s.x1["full"].tobytes()
        assert ctx.frames_count() == s.rec1["full"].size
        _check_records(_frames_once(ctx), s.rec1["full"])
        _check_diag(ctx.diag(CN), s.diag1["full"], DIAG_STREAM)
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), s.rec0)
        ctx.upload_wait()
    finally:
        ctx.close()


def test_generator_refuses_where_the_download_does(voice):
    """A context whose only input is a staged one that has not run: m17hip_download_i16 is M17HIP_ESTATE, so is the generator, and nothing is written."""
    s = voice
    ctx = tx_context(maxT=T1)
    try:
        ctx.upload_async(s.pin1["full"].data_ptr(), CN, T1)
        _refused(ctx, T1, "a staged input alone")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- B3 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_generator_under_tuning_key_16(voice, blocks):
    """Tuning key 16 = 1: m17hip_upload_i16 writes the STAGING slab.  Before its run the generator follows m17hip_download_i16 exactly — refused while the
    context has run nothing, the slab of the run before afterwards —; behind the run (in flight: asserted) it modulates the new input.  A TX context under
    key 16 cannot modulate what it has just uploaded or synthesised until a run has been made."""
    s = voice
    m = _behind(blocks)
    again = m.block(s.x0)
    nxt = m.block(s.x1["full"])
    t1, t3 = _out(T0), _out(T1)
    ctx = tx_context(keys=(16,))
    try:
        ctx.upload(s.x0)
        _refused(ctx, T0, "key 16: the first input is in the staging slab")
        ctx.run(channels=CN, samples=T0)
        _in_flight(ctx)
        _generate(ctx, "device", T0, "behind the first run under key 16", blocks["first"], t1)
        ctx.upload(s.x1["full"])
        code, rows = _download(ctx, T0)
        assert code == 0 and np.array_equal(rows, s.x0), "the current slab is still run 0's"
        _generate(ctx, "host", T0, "key 16: the slab of the run before, not what was just uploaded", again)
        ctx.run(channels=CN, samples=T1)
        _in_flight(ctx, "run 1")
        _generate(ctx, "device", T1, "behind the second run under key 16", nxt, t3)
        _check_records(_frames_once(ctx), s.rec1["full"])
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), s.rec0)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- B4 -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_table_at_once_with_a_run_in_flight(voice, blocks):
    """m17hip_synth_wide_channels with run 0 in flight never waits (the run is still in flight when it has returned), and the next block follows the new
    table: a channel that was silent in block 1 is audible in block 2 with block 1's integral in its phase base, another has moved."""
    s = voice
    m = _behind(blocks)
    assert int(m.a2[LATE]) != 0 and int(m.last[LATE]) == int(s.x0[LATE, -1])
    m.channels(*table(late=True))
    exp = m.block(s.x0)
    zero = _behind(blocks)
    zero.channels(*table(late=True))
    zero.a2[LATE], zero.last[LATE] = 0, 0
    other = zero.block(s.x0)
    assert (exp[1] != other[1]).any() and np.array_equal(exp[0], other[0]), "the silent channel's carry decides its source's bytes"
    t1, t2 = _out(T0), _out(T0)
    ctx = tx_context()
    try:
        ctx.upload_device(s.dev.data_ptr(), CN, T0, pitch=T0 + T1)
        _generate(ctx, "device", T0, "block 1", blocks["first"], t1)
        ctx.run()
        _in_flight(ctx)
        ctx.synth_wide_channels(*table(late=True))
        _in_flight(ctx, "run 0 (after m17hip_synth_wide_channels has returned)")
        _generate(ctx, "device", T0, "block 2 under the new table", exp, t2)
        _run_0_is(ctx, s)
    finally:
        ctx.close()


def test_configuration_at_once_with_a_run_in_flight(voice, blocks):
    """m17hip_synth_wide_config, then the table, with run 0 in flight: neither waits; the next block is a fresh feed of the new configuration."""
    s = voice
    first = 35 * GP
    exp = host_form(sigma=20.0, seed=99, first=first, late=True).block(s.x0)
    t1, t2 = _out(T0), _out(T0)
    ctx = tx_context()
    try:
        ctx.upload_device(s.dev.data_ptr(), CN, T0, pitch=T0 + T1)
        _generate(ctx, "device", T0, "block 1", blocks["first"], t1)
        ctx.run()
        _in_flight(ctx)
        ctx.synth_wide_config(GS, GP, GQ, GFMT, None, 20.0, 99, first)
        _in_flight(ctx, "run 0 (after m17hip_synth_wide_config has returned)")
        ctx.synth_wide_channels(*table(late=True))
        _in_flight(ctx, "run 0 (after m17hip_synth_wide_channels has returned)")
        _generate(ctx, "device", T0, "block 2, a fresh feed of the new configuration", exp, t2)
        _run_0_is(ctx, s)
    finally:
        ctx.close()


def test_reset_of_the_tx_context_with_a_run_in_flight(voice, blocks):
    """m17hip_demod_reset on the TX context with run 0 in flight: the next block is a fresh feed's, at the configuration's first_sample."""
    s = voice
    first = 11 * GP
    m = host_form(first=first)
    one = m.block(s.x0)
    continued = m.block(s.x0)
    m.reset()
    assert m.count == first
    exp = m.block(s.x0)
    assert exp.tobytes() == one.tobytes() and all((continued[k, :5] != exp[k, :5]).any() for k in range(GS)), "a feed that went on has other bytes"
    t1, t2 = _out(T0), _out(T0)
    ctx = tx_context(first=first)
    try:
        ctx.upload_device(s.dev.data_ptr(), CN, T0, pitch=T0 + T1)
        _generate(ctx, "device", T0, "block 1", one, t1)
        ctx.run()
        _in_flight(ctx)
        ctx.reset()
        _generate(ctx, "device", T0, "a fresh feed behind the reset", exp, t2)
    finally:
        ctx.close()


# ---- B5: TX feeds RX through two device buffers, block after block -------------------------------------------------------------------------------------------
S5, PER5 = p2.S, p2.PER_SOURCE
C5 = S5 * PER5
LENS = (pr.T1, TB, TB, pr.T1)                       # outputs of the four blocks
CUTS = np.cumsum((0,) + LENS).tolist()
A5, SEED5 = 6000.0, 5
RX = {"resample": dict(P=pr.R1 * pr.D, Q=pr.U, sigma=float(cpu.SIGMA), fcw=pr.FCW, ratio=pr.RATIO),
      "wide2": dict(P=p2.R, Q=1, sigma=float(p2.SIGMA[wl.IQ_I16]), fcw=p2.FCW, ratio=float(p2.R))}
assert pr.T1 == p2.T1 and pr.OFFSETS == p2.OFFSETS and all(n % pr.U == 0 for n in LENS)


class Link:
    """One receiver's side of B5, all of it on the CPU: the basebands, the host form's multiplex of the four blocks, the parents' feeds over those bytes
    block by block, and the float oracle's records on the floats."""

    def __init__(self, kind):
        r = RX[kind]
        self.kind, self.P, self.Q, self.sigma = kind, r["P"], r["Q"], r["sigma"]
        total = CUTS[-1]
        p = ol.gen_params(seed=20261020, kind=-1, n_frames=max(total // 1920 - 3, 1), lead_in=48, total=total)
        self.bb = ol.generate_batch(p, C5, total, threads=po.THREADS)
        self.src = np.repeat(np.arange(S5, dtype=np.uint32), PER5)   # (transmission k of source s is baseband row PER_SOURCE * s + k, as in the parents)
        self.fcw = [m17hip.wide_fcw(p2.OFFSETS[c % PER5], r["ratio"]) for c in range(C5)]
        mux = wt.Mux(S5, self.P, self.Q, wt.k_stated(self.P), wt.IQ_I16, self.sigma, SEED5, 0, channels=C5)
        mux.channels(self.src, self.fcw, 0, A5)
        self.wide = [mux.block(self.bb[:, a:b]) for a, b in zip(CUTS[:-1], CUTS[1:])]
        x = np.concatenate(self.wide, axis=1)
        clipped = float(((x == -32768) | (x == 32767)).any(axis=-1).mean())
        assert clipped <= cpu.CLIPPED_CAP, clipped
        assert PER5 * A5 + 8.0 * self.sigma <= 32767.0
        f = pr.feeds(x) if kind == "resample" else p2.feeds(x)
        self.y = [f.block(a, b) for a, b in zip(CUTS[:-1], CUTS[1:])]
        assert all(np.isfinite(y).all() for y in self.y)
        e = Expect(np.ascontiguousarray(np.concatenate(self.y, axis=1)))
        self.recs = [rep_rows(e.run(a, b)) for a, b in zip(CUTS[:-1], CUTS[1:])]
        self.diags = rep(e.diags)
        assert sum(r.size for r in self.recs) > ALL, "the expectation holds records"
        self.rows = lambda n: n // self.Q * self.P


@pytest.fixture(scope="module")
def links():
    return {}


def _link(links, kind):
    if kind not in links:
        links[kind] = Link(kind)
    return links[kind]


def _rx_records_once(rx):
    return pr._frames_once(rx)


@pytest.mark.parametrize("buffers", [2, 1], ids=["two_buffers", "one_buffer"])
@pytest.mark.parametrize("kind", ["resample", "wide2"])
def test_tx_feeds_rx_block_after_block(request, links, kind, buffers):
    """Per block: the next baseband rows uploaded into the TX context in place, m17hip_synth_wide_device into buf[n % 2], the RX context's
    m17hip_upload_wide_device_async of that buffer, its run.  The RX floats of every block are the parents' feeds' over the host form's multiplex, both
    sides' carries crossing four blocks, and every run's records and the final m17_diag the float oracle's on those floats.

    What synchronises: m17hip_upload_wait on the RX context before a buffer is written a second time (the caller's duty by the header), and the fetches
    this test itself makes — block n's floats are downloaded behind block n + 1's staging, in front of its run, and run n's records behind run n + 1's
    queueing.  Block 2's TX upload and generator call are made while block 1's tuner is still in flight (the parents' premise, asserted).  Behind them
    every download has waited for a run, and with it for that block's tuner, and m17hip_upload_wait has drained the copy stream in front of blocks 3 and
    4: for those the intervals are printed and nothing about them can be asserted.  With one buffer and m17hip_upload_wait behind every staging the words
    are the same."""
    import torch
    L = _link(links, kind)
    if kind == "resample":
        request.getfixturevalue("case")
        Dt = request.getfixturevalue("tuner_resample_s")
        rx = pr.context()
    else:
        Dt = request.getfixturevalue("tuner_wide2_s")["i16"]
        rx = p2.context(wl.IQ_I16)
    pitch = L.rows(max(LENS))
    bufs = [torch.full((S5, pitch, 2), 77, dtype=torch.int16, device="cuda") for _ in range(buffers)]
    torch.cuda.synchronize()
    tx = m17hip.Context(C5, max(LENS))
    try:
        tx.synth_wide_config(S5, L.P, L.Q, wt.IQ_I16, None, L.sigma, SEED5, 0)
        tx.synth_wide_channels(L.src, L.fcw, 0, A5)
        t_s = None
        for n, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
            buf = bufs[n % buffers]
            if n == 1 and buffers == 2:
                _made_under_the_tuner(t_s, Dt, f"block 2's m17hip_upload_i16 on the TX context ({kind})")
            elif n:
                print(f"[wide_tx] block {n + 1}'s TX upload: {1e3 * (time.perf_counter() - t_s):.3f} ms after the staging call before it began")
            tx.upload(L.bb[:, a:b])
            if n >= buffers:
                rx.upload_wait()
            if n == 1 and buffers == 2:
                _made_under_the_tuner(t_s, Dt, f"block 2's m17hip_synth_wide_device ({kind})")
            elif n:
                print(f"[wide_tx] block {n + 1}'s generator call: {1e3 * (time.perf_counter() - t_s):.3f} ms after the staging call before it began")
            tx.synth_wide(out=buf)
            t_s = time.perf_counter()
            rx.upload_wide_device_async(buf.data_ptr(), ALL, b - a, pitch, p2.GAIN)
            if buffers == 1:
                rx.upload_wait()
            if n:
                rx.T = LENS[n - 1]
                _check_words(rx.download_f32(), rep(L.y[n - 1]), f"the floats of block {n} ({kind})")
            rx.run(channels=ALL, samples=b - a)
            if n:
                rx.frames_select(1)
                _check_records(_rx_records_once(rx), L.recs[n - 1])
                rx.frames_select(0)
        rx.T = LENS[-1]
        _check_words(rx.download_f32(), rep(L.y[-1]), f"the floats of block {len(LENS)} ({kind})")
        _check_records(_rx_records_once(rx), L.recs[-1])
        _check_diag(rx.diag(ALL), L.diags, DIAG_STREAM)
        rx.upload_wait()
        for n in range(len(LENS) - buffers, len(LENS)):   # (the blocks the buffers still hold: no byte of a buffer is read by this test before)
            got = np.ascontiguousarray(bufs[n % buffers][:, : L.rows(LENS[n])].cpu().numpy())
            _same(got, L.wide[n], f"the multiplex of block {n + 1} ({kind})")
    finally:
        tx.close()
        rx.close()
        torch.cuda.synchronize()
