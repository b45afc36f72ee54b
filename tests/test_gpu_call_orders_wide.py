"""GPU tests of the host-side call orders of wideband IQ input (ABI 609: m17hip_wide_config, m17hip_wide_channels, m17hip_upload_wide and friends) with a
run STILL IN FLIGHT: the regime of tests/test_gpu_call_orders_formats.py as it stands (a fresh context per case, run 0 queued, the call under test made at
once with nothing synchronising in between, every comparison exact) for the cross-stream paths the tuner added — the channel table in a turn-taking pair
of device copies with the main and the copy stream as readers, the sources' histories in two copies that take turns and that only one event orders between
the two streams, one z buffer shared by both, the histories zeroed on the stream of the latest IQ launch, m17hip_wide_config waiting for the tuner in
flight before it reallocates, the host forms' raw buffer (sized by sources) growing while the block before may still be read.

What is compared: the floats (m17hip_download_f32) as uint32 words against the HOST form fed block by block (wide_lib.Tuner / wide_lib.Feeds: histories,
count and carries are the feed's); records, m17_diag and counts byte for byte against the float oracle stepped on the host form's floats.

Shape: 64 channels on two sources at R = 2 (96 kSPS), 33 taps (a Hamming-windowed sinc, cutoff 7 kHz: the smallest odd length whose stop band begins
inside the 24 kHz between two transmissions); per source four FM transmissions from wide_lib.wideband; 32 channels per source, eight per transmission, each
a few Hz beside the next so that no two channels share a frequency word.  Run 0 = 96 000 outputs, run 1 = one frame ("tiny", 1920) or 24 000 ("full").
The run length was chosen by the parent module's rule from a measurement on the MI355X (a throwaway context first; fresh contexts throughout; from the
return of m17hip_demod_run to the end of its work on the main stream, six contexts per producer and format; the host-side duration of every staging
call the cases use, three contexts each, int16 and uint8):
    run 0 at 64 x  96 000:  3.61 - 3.71 ms in flight   longest staging 0.40 ms   ratio 9.0
The smallest of 96 000, 192 000 and 480 000 whose shortest in-flight time is at least four times the longest staging time is taken: 96 000, the first
of them, so the longer ones were not measured.  The tuner in front does not show in the in-flight time (the parent measured 3.66 - 3.80 ms for the
chain alone: the tuner's 64 x 96 000 outputs at 33 taps have left the device before m17hip_demod_run returns, the in-place forms wait for them).  The
stagings: from pinned memory 0.11 - 0.13 ms, from device memory 0.10 - 0.12 ms, tuning key 16 with an in-place upload 0.21 - 0.40 ms (it waits for
its own tuner), a retune and the staged block that publishes it, the second table copy's allocation included, 0.12 - 0.17 ms.  A full run 1 queued
behind run 0 has 0.02 ms left once run 0's records have been fetched: a premise can only be asserted directly behind m17hip_demod_run, which is where
every case asserts it.
Beyond the margin every case asserts its own premise with the parent's _in_flight just before the call under test: a case whose run 0 had already
finished FAILS.
"""
import copy
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import iq_lib as iq
import m17hip
import oracle_lib as ol
import test_gpu_call_orders_formats as par
import wide_lib as wl
from test_gpu_call_orders_formats import (AFTERS, CHUNK, CN, DIAG_STREAM, FEED_AGAIN, FEED_CUTS, FEED_HOW, FEED_LEN, FEED_RESET_AFTER, FETCHES, LEN, STAGES, T0, T1,
                                          THREADS, TINY, Expect, Runs, _call, _check_diag, _check_records, _check_words, _compact_device, _frames_once,
                                          _in_flight, _matrix, _rec_cap, _then, _u32)

pytestmark = pytest.mark.gpu

S, R, L = 2, 2, 33
PER_SOURCE = 4
OFFSETS = (-36000.0, -12000.0, 12000.0, 36000.0)   # Hz from the source's centre: 24 kHz apart, inside the +-48 kHz a source covers
STEP_HZ = 3.0                                      # the j-th listener to a transmission's offset, on either source, listens j * STEP_HZ beside it: another word, the same frames
FMTS = {"i16": wl.IQ_I16, "u8": wl.IQ_U8}
AMPLITUDE = {wl.IQ_I16: 6000.0, wl.IQ_U8: 28.0}    # (four carriers of 28 stay inside a byte)
SIGMA = {wl.IQ_I16: 300.0, wl.IQ_U8: 0.0}
SB = {wl.IQ_I16: 4, wl.IQ_U8: 2}
GAIN = 1.0
SRC = np.array([c % S for c in range(CN)], dtype=np.uint32)
TX = np.array([(c // S) % PER_SOURCE for c in range(CN)])
FCW = np.array([m17hip.wide_fcw(OFFSETS[TX[c]] + STEP_HZ * (c // (S * PER_SOURCE) + 8 * SRC[c]), R) for c in range(CN)], dtype=np.int64)
assert len(set(FCW.tolist())) == CN, "no two channels share a frequency word"
# the generator alternates BERT (even rows) and stream (odd rows); transmission k of source s is baseband row PER_SOURCE * s + k
GROUPS = {"bert": [c for c in range(CN) if (PER_SOURCE * SRC[c] + TX[c]) % 2 == 0], "stream": [c for c in range(CN) if (PER_SOURCE * SRC[c] + TX[c]) % 2 == 1]}


def taps():
    t = np.arange(L, dtype=np.float64) - 0.5 * (L - 1)
    h = np.sinc(2.0 * 7000.0 / (48000.0 * R) * t) * (0.54 + 0.46 * np.cos(2.0 * np.pi * t / (L - 1)))
    return (h / h.sum()).astype(np.float32)


TAPS = taps()


def sources(total, fmt, seed=20261019):
    """x[S] source rows of total * R samples: PER_SOURCE transmissions each (BERT and stream by turns, as long as the row)."""
    p = ol.gen_params(seed=seed, kind=-1, n_frames=total // 1920 - 7, lead_in=3072, total=total)
    bb = ol.generate_batch(p, S * PER_SOURCE, total, threads=THREADS)
    x = np.stack([wl.wideband(bb[PER_SOURCE * s: PER_SOURCE * (s + 1)], OFFSETS, R, amplitude=AMPLITUDE[fmt], sigma=SIGMA[fmt], seed=s + 1, fmt=fmt) for s in range(S)])
    x.setflags(write=False)
    return x


def _pool(fn, n):
    wl.lib(), iq.lib()   # (built on first use: by one thread, before sixteen ask for them)
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, range(n)))


class PFeeds(wl.Feeds):
    """wide_lib.Feeds with the channels of a block on a thread pool (the host form is called through ctypes: the threads run side by side)."""

    def block(self, a, b):
        def one(c):
            s = self.src[c]
            t = wl.Tuner(self.taps, self.R, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            out = t.block(self.data[s][a * self.R: b * self.R])
            return out, t.carry
        res = _pool(one, len(self.src))
        for c, (_, carry) in enumerate(res):
            self.carry[c] = carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][a * self.R: b * self.R])
        return np.stack([o for o, _ in res])


def wide_stream(fmt):
    """The sources, and per channel the host form fed block by block: block 0 = run 0's outputs, block 1 the tiny or the full chunk behind it, with the
    history, count and carry block 0 left.  The float oracle's verdict on those floats."""
    x = sources(T0 + T1, fmt)
    ref = PFeeds(x, TAPS, SRC, FCW, R, GAIN)
    y0 = ref.block(0, T0)
    y1 = {name: copy.deepcopy(ref).block(T0, T0 + t) for name, t in LEN.items()}
    assert np.array_equal(_u32(y1["tiny"]), _u32(y1["full"][:, :TINY]))
    y = np.concatenate([y0, y1["full"]], axis=1)
    assert np.isfinite(y).all()
    fresh = PFeeds(x[:, T0 * R:], TAPS, SRC, FCW, R, GAIN).block(0, 4)
    assert (_u32(fresh[:, 0]) != _u32(y[:, T0])).all() and (_u32(fresh[:, 1:]) != _u32(y[:, T0 + 1:T0 + 4])).any(), "block 1's first floats are the ones the carry and the history decide"
    runs = Runs(y)
    runs.assert_records_in_both_runs(GROUPS)
    return x, y, runs, ref


class Buffers:
    """The sources as run 0's block and the two chunks behind it: in host memory, pinned, on the device."""

    def __init__(self, fmt, x, y, runs, ref):
        import torch
        self.fmt, self.x, self.y, self.runs, self.ref = fmt, x, y, runs, ref
        self.sb = SB[fmt]
        self.x0 = np.ascontiguousarray(x[:, :T0 * R])
        self.x1 = {"full": np.ascontiguousarray(x[:, T0 * R:]), "tiny": np.ascontiguousarray(x[:, T0 * R:(T0 + TINY) * R])}
        self.pin1 = {k: torch.from_numpy(v).pin_memory() for k, v in self.x1.items()}
        self.dev = torch.from_numpy(np.array(x)).cuda()   # (a writable copy: the fixtures are read-only)
        self.recbuf = torch.empty(CN * _rec_cap(T0 + T1) * m17hip.FRAME_REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                         # (the producers' buffers are complete before they are handed over: include/m17hip.h)
        self.pitch = (T0 + T1) * R
        self.dev1 = self.dev.data_ptr() + self.sb * T0 * R


def context(fmt, maxT=T0, src=SRC, fcw=FCW):
    ctx = m17hip.Context(CN, maxT)
    ctx.wide_config(S, R, fmt, TAPS)
    ctx.wide_channels(src, fcw)
    return ctx


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def first_staging_of_the_process():
    """The parent module's throwaway context and staging (the first staging of a process costs about 15 ms in allocations), and one wideband block and
    one retune: the pinned staging of a channel table and its device copies have been allocated once in this process before any case allocates its own."""
    import torch
    x = np.zeros((CN, 2 * TINY), dtype=np.int16)
    pin = torch.from_numpy(x.copy()).pin_memory()
    ctx = m17hip.Context(CN, 2 * TINY)
    try:
        ctx.upload(x)
        ctx.run()
        ctx.upload_async(pin.data_ptr(), CN, 2 * TINY)
        ctx.run(channels=CN, samples=2 * TINY)
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()
    w = np.zeros((S, 2 * TINY * R, 2), dtype=np.int16)
    wpin = torch.from_numpy(w.copy()).pin_memory()
    ctx = context(wl.IQ_I16, 2 * TINY)
    try:
        ctx.upload_wide(w)
        ctx.run()
        ctx.wide_channels(SRC[::-1].copy(), FCW)
        ctx.upload_wide_async(wpin.data_ptr(), CN, 2 * TINY, 2 * TINY * R)
        ctx.run(channels=CN, samples=2 * TINY)
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def wide_cases():
    return {name: Buffers(f, *wide_stream(f)) for name, f in FMTS.items()}


# ---- the steps of a case -------------------------------------------------------------------------------------------------------------------------
PRODUCERS = ("upload_wide", "upload_wide_device")


def _produce(ctx, b, producer):
    """Run 0's input, tuned in place."""
    if producer == "upload_wide":
        ctx.upload_wide(b.x0, gain=GAIN)
    else:
        ctx.upload_wide_device(b.dev.data_ptr(), CN, T0, b.pitch, GAIN)


def _stage(ctx, b, stage):
    """The context's first staged input: the chunk behind run 0, tuned on the copy stream."""
    chunk = CHUNK[stage]
    t = LEN[chunk]
    if stage in ("async_tiny", "async_full"):
        ctx.upload_wide_async(b.pin1[chunk].data_ptr(), CN, t, t * R, GAIN)
    elif stage == "device_async":
        ctx.upload_wide_device_async(b.dev1, CN, t, b.pitch, GAIN)
    else:
        ctx.tune(16, 1)
        ctx.upload_wide(b.x1[chunk], gain=GAIN)


def _words(b, chunk):
    return b.y[:, T0:T0 + LEN[chunk]]


def _after_run_1(ctx, b, chunk):
    """Run 1 was queued: every fetch once more, and the floats it read."""
    r = b.runs
    ctx.frames_select(1)
    _check_records(_frames_once(ctx), r.rec0)
    ctx.frames_select(0)
    assert ctx.frames_count() == r.rec1[chunk].size
    _check_records(_frames_once(ctx), r.rec1[chunk])
    _check_records(_compact_device(ctx, b), r.rec1[chunk])
    _check_diag(ctx.diag(CN), r.diag1[chunk], DIAG_STREAM)
    _check_words(ctx.download_f32(), _words(b, chunk), "the floats run 1 read")


def _case(b, producer, stage, call, after):
    ctx = context(b.fmt)
    try:
        chunk = CHUNK[stage]
        t = LEN[chunk]
        _produce(ctx, b, producer)
        ctx.run()
        _stage(ctx, b, stage)                            # run 0 is still on the device: nothing in between synchronises
        _then(ctx, after, t)
        _call(ctx, b, call, after, chunk)
        if after != "run_select1":
            ctx.run(channels=CN, samples=t)
        _after_run_1(ctx, b, chunk)
        ctx.upload_wait()
    finally:
        ctx.close()


def test_the_matrices_meet_every_producer_and_staging():
    """(No GPU work.)  The rotation reaches every (producer, staging) pair, per format, and every call and what follows the staging; the other families
    of cases are all there."""
    for fmt in FMTS:
        mine = [p.values for p in _matrix(FETCHES, PRODUCERS, tuple(FMTS)) if p.values[0] == fmt]
        assert set(v[1:3] for v in mine) == set(itertools.product(PRODUCERS, STAGES))
        assert set(v[3:5] for v in mine) == set(itertools.product(FETCHES, AFTERS))
    assert FETCHES == ("frames_count", "frames", "compact_device", "diag") and AFTERS == ("direct", "front", "run_select1")
    assert STAGES == ("async_tiny", "async_full", "device_async", "tune16_upload")
    assert set(FEED_HOW) == {"pinned", "host", "device"} and len(FEED_HOW) == 6
    assert len(RETUNES) == 4 and len(RETUNE_HOW["in_place_first"]) >= 5 and set(RETUNE_HOW["in_place_first"]) == set(RETUNE_HOW["staged_first"]) == {"in_place", "pinned", "device"}


# ---- 1: a fetch right after the first wideband staging ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,producer,stage,call,after", _matrix(FETCHES, PRODUCERS, tuple(FMTS)))
def test_fetch_right_after_the_first_wideband_staging(wide_cases, fmt, producer, stage, call, after):
    """Run 0's block tuned in place on the main stream (its channel table published there), the next block staged at once: its tuner runs on the copy
    stream, behind the table's `ready`, the carries, the z buffer and the histories the main stream's launch left (from host memory also the raw buffer) —
    then the fetch, which names run 0.  After run 1 the floats of its block are the host form's for block 1 of the feed."""
    _case(wide_cases[fmt], producer, stage, call, after)


# ---- 2: an in-place wideband upload with run 0 in flight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("form", ["host", "device"])
def test_in_place_wideband_upload_with_run_0_in_flight(wide_cases, form, fmt):
    """No staging at all: the tuner of block 1 writes the float slab run 0 still reads."""
    b, r = wide_cases[fmt], wide_cases[fmt].runs
    ctx = context(b.fmt)
    try:
        _produce(ctx, b, PRODUCERS[form == "device"])
        ctx.run()
        _in_flight(ctx)
        if form == "host":
            ctx.upload_wide(b.x1["full"], gain=GAIN)
        else:
            ctx.upload_wide_device(b.dev1, CN, T1, b.pitch, GAIN)
        _check_words(ctx.download_f32(), _words(b, "full"), "the floats run 1 reads")
        ctx.run()
        _check_records(_frames_once(ctx), r.rec1["full"])
        _check_diag(ctx.diag(CN), r.diag1["full"], DIAG_STREAM)
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), r.rec0)
    finally:
        ctx.close()


# ---- 3: retunes with work in flight ----------------------------------------------------------------------------------------------------------------
# block 0 is run 0's (T0 outputs); five more of 4800 outputs each lie behind it in the full chunk: six in all
RT_LEN = (T0,) + (T1 // 5,) * 5
RT_CUTS = np.concatenate([[0], np.cumsum(RT_LEN)]).tolist()
RETUNE_HOW = {"in_place_first": ("in_place", "pinned", "in_place", "device", "in_place", "pinned"),
              "staged_first": ("in_place", "device", "pinned", "in_place", "device", "in_place")}


def _tables():
    """Tables 1 .. 4: each moves another quarter of the channels to the other source, to the word of another transmission there, 50 Hz and more beside
    every word in use (so still no two channels share one).  (who moved, source[CN], fcw[CN]) per table."""
    out, src, fcw = [], SRC.copy(), FCW.copy()
    for k in range(4):
        who = np.arange(k, CN, 4)
        src, fcw = src.copy(), fcw.copy()
        src[who] = 1 - src[who]
        fcw[who] = [m17hip.wide_fcw(OFFSETS[(TX[c] + 1 + k) % PER_SOURCE] + 50.0 + STEP_HZ * c, R) for c in who]
        assert len(set(fcw.tolist())) == CN
        out.append((who, src, fcw))
    return out


RETUNES = _tables()


@pytest.mark.parametrize("order", list(RETUNE_HOW))
def test_retunes_with_work_in_flight(wide_cases, order):
    """m17hip_wide_channels at once after run 0 was queued — the block behind it, staged, publishes the new table on the copy stream into the second
    device copy, which this context allocates there and then (the premise is asserted before the call); a second retune at once behind that staged block
    and before its run: the staged block keeps its table, the next block in place on the main stream has the new one; a third and a fourth, so that each
    device copy is rewritten after blocks tuned with it were queued on either stream.  Every block's floats are the host form's under the table in force at
    its upload; a channel's first output behind a retune is taken against the carry it had (include/m17hip.h)."""
    b = wide_cases["i16"]
    how = RETUNE_HOW[order]
    ref = PFeeds(b.x, TAPS, SRC, FCW, R, GAIN)
    pin = b.pin1["full"]
    ctx = context(b.fmt)
    try:
        def up(k):
            a, n = RT_CUTS[k], RT_LEN[k]
            if how[k] == "in_place":
                ctx.upload_wide_device(b.dev.data_ptr() + a * R * b.sb, CN, n, b.pitch, GAIN)
            elif how[k] == "device":
                ctx.upload_wide_device_async(b.dev.data_ptr() + a * R * b.sb, CN, n, b.pitch, GAIN)
            else:
                ctx.upload_wide_async(pin.data_ptr() + (a - T0) * R * b.sb, CN, n, T1 * R, GAIN)
            return ref.block(a, a + n)

        def settle(k, e):
            if how[k] != "in_place":
                ctx.run(channels=CN, samples=RT_LEN[k])
            _check_words(ctx.download_f32(), e, f"floats of block {k} ({how[k]})")
            if how[k] == "in_place":
                ctx.run()

        def retune(k):
            _, src, fcw = RETUNES[k]
            ctx.wide_channels(src, fcw)
            ref.src, ref.fcw = list(src), list(fcw)

        e0 = up(0)
        ctx.run()
        _in_flight(ctx)
        retune(0)                                        # at once after run 0 was queued
        e1 = up(1)                                       # staged: the new table goes to the device on the copy stream
        retune(1)                                        # at once behind the staged block, before its run: block 1 keeps table 1
        settle(1, e1)
        assert not np.array_equal(_u32(e1), _u32(b.y[:, RT_CUTS[1]:RT_CUTS[2]]))
        e2 = up(2)                                       # under table 2
        if how[2] != "in_place":
            retune(2)                                    # (behind a staged block once more)
            settle(2, e2)
        else:
            settle(2, e2)
            retune(2)                                    # with run 2 queued
        e3 = up(3)
        if how[3] != "in_place":
            retune(3)
            settle(3, e3)
        else:
            settle(3, e3)
            retune(3)
        for k in (4, 5):
            settle(k, up(k))
        moved, _, _ = RETUNES[0]
        assert (_u32(e1[moved]) != _u32(b.y[moved, RT_CUTS[1]:RT_CUTS[2]])).any(axis=1).all()
        ctx.upload_wait()
    finally:
        ctx.close()
    assert np.array_equal(_u32(e0), _u32(b.y[:, :T0]))


# ---- 4: a live wideband feed -------------------------------------------------------------------------------------------------------------------------
# the parent's six blocks (pinned, host, device by turns; blocks 1 and 3 come from host memory and are longer than all before them: the raw buffer, sized
# by sources, grows while the block before may still be read).  m17hip_demod_reset_channels for a third of the channels at once after run 1 was queued;
# m17hip_demod_reset behind run 2; m17hip_wide_config again behind run 3, whose block was staged
FEED_FULL_RESET_AFTER = 2
FEED_SEED = 20261024   # the first generator seed from 20261019 on with which every channel, in both formats, yields records before the listed ones start over
FEED_CONFIG_AFTER = 3
assert FEED_RESET_AFTER == 1 and FEED_HOW[FEED_CONFIG_AFTER] == "pinned"


def feed_case(fmt):
    """The floats of every block from the Feeds model — the listed channels' carries zeroed behind block 1, a fresh host form on the same table from block 3,
    the sources started over with the carries kept from block 4 — and the float oracle's records run by run: the listed channels' restart at block 2,
    every channel's at block 3 (where the context's stream begins again at sample 0)."""
    x = sources(FEED_CUTS[-1], fmt, seed=FEED_SEED)
    cut = lambda k: FEED_CUTS[k]
    ref = PFeeds(x, TAPS, SRC, FCW, R, GAIN)
    ys = [ref.block(cut(0), cut(1)), ref.block(cut(1), cut(2))]
    for c in FEED_AGAIN:
        ref.carry[c] = np.zeros(2, dtype=np.float32)
    ys.append(ref.block(cut(2), cut(3)))
    assert (ys[2][FEED_AGAIN, 0] == 0).all() and (np.delete(ys[2][:, 0], FEED_AGAIN) != 0).all()
    fresh = PFeeds(x[:, cut(3) * R:], TAPS, SRC, FCW, R, GAIN)
    ys.append(fresh.block(0, FEED_LEN[3]))
    assert not np.array_equal(_u32(ys[3][:, :8]), _u32(ref.block(cut(3), cut(3) + 8)))
    again = PFeeds(x[:, cut(4) * R:], TAPS, SRC, FCW, R, GAIN)
    again.carry = [c.copy() for c in fresh.carry]
    ys.append(again.block(0, FEED_LEN[4]))
    assert not np.array_equal(_u32(ys[4][:, :8]), _u32(fresh.block(FEED_LEN[3], FEED_LEN[3] + 8)))
    ys.append(again.block(FEED_LEN[4], FEED_LEN[4] + FEED_LEN[5]))
    # the records: blocks 0 .. 2 are one stream (the listed channels start over at block 2), blocks 3 .. 5 another
    ya, yb = np.concatenate(ys[:3], axis=1), np.concatenate(ys[3:], axis=1)
    at = cut(2)
    origin = np.zeros(CN, dtype=np.int64)
    origin[FEED_AGAIN] = at
    exp_a = Expect(ya, origin=origin)
    first = Expect(np.ascontiguousarray(ya[FEED_AGAIN, :at]))
    exp_b = Expect(yb)
    rows = []
    for k in range(6):
        if k < 3:
            r = exp_a.run(cut(k), cut(k + 1))
            if k <= FEED_RESET_AFTER:
                f = first.run(cut(k), cut(k + 1))
                for i, c in enumerate(FEED_AGAIN):
                    r[c] = f[i]
                    r[c]["channel"] = c
        else:
            r = exp_b.run(cut(k) - cut(3), cut(k + 1) - cut(3))
        assert sum(q.size for q in r) > CN, f"run {k} yields records"
        rows.append(np.concatenate(r))
    after = exp_a.run(at, cut(3))
    # (one block of 24 000 samples, joined in mid-transmission: a BERT channel yields one record there, a stream channel ten)
    seen = [c for c in FEED_AGAIN if after[c].size > 0]
    assert len(seen) >= 3 * len(FEED_AGAIN) // 4 and all(after[c]["seq"][0] == 0 for c in seen), "the listed channels' records restart"
    assert all(first.recs[i].size > 0 for i in range(len(FEED_AGAIN))), "... after those of their first stream"
    return x, ys, rows, exp_b.diags


@pytest.fixture(scope="module")
def feed_cases():
    import torch
    out = {}
    for name, f in FMTS.items():
        x, ys, rows, diags = feed_case(f)
        pin, dev = torch.from_numpy(np.array(x)).pin_memory(), torch.from_numpy(np.array(x)).cuda()
        torch.cuda.synchronize()
        out[name] = (x, ys, rows, diags, pin, dev)
    return out


def _feed_block(ctx, x, pin, dev, f, k):
    a, n, sb, pitch = FEED_CUTS[k] * R, FEED_LEN[k], SB[f], FEED_CUTS[-1] * R
    if FEED_HOW[k] == "pinned":
        ctx.upload_wide_async(pin.data_ptr() + a * sb, CN, n, pitch, GAIN)
    elif FEED_HOW[k] == "host":
        ctx.upload_wide(x[:, a:a + n * R], gain=GAIN)
    else:
        ctx.upload_wide_device_async(dev.data_ptr() + a * sb, CN, n, pitch, GAIN)


@pytest.mark.parametrize("check", ["records_behind_the_next_run", "floats_and_records_run_by_run"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_live_wideband_feed(feed_cases, fmt, check):
    """Six blocks with no host synchronisation beyond what the calls themselves do.  `records_behind_the_next_run`: run k's records are fetched behind run
    k + 1 and only the in-place blocks' floats are read back, so the device never drains — m17hip_demod_reset is made with run 2 in flight (asserted, so
    directly behind m17hip_demod_run: the records of runs 1 and 2 are given up, as include/m17hip.h says) and m17hip_wide_config with run 3, whose block
    was staged, in flight (asserted as well).  The other order
    reads every block's floats and every run's records, run 2's before the reset."""
    x, ys, rows, diags, pin, dev = feed_cases[fmt]
    f = FMTS[fmt]
    live = check == "records_behind_the_next_run"
    ctx = context(f, max(FEED_LEN))
    try:
        for k, n in enumerate(FEED_LEN):
            _feed_block(ctx, x, pin, dev, f, k)
            if FEED_HOW[k] == "host":
                _check_words(ctx.download_f32(), ys[k], f"floats of block {k}")
            ctx.run(channels=CN, samples=n)
            if k == FEED_RESET_AFTER:
                _in_flight(ctx, f"run {k}")
                ctx.reset_channels(FEED_AGAIN)
            if live:
                if k > 0 and k != FEED_FULL_RESET_AFTER and k - 1 != FEED_FULL_RESET_AFTER:
                    ctx.frames_select(1)
                    _check_records(_frames_once(ctx), rows[k - 1])
                    ctx.frames_select(0)
                if k == FEED_FULL_RESET_AFTER:
                    _in_flight(ctx, f"run {k}")
                    ctx.reset()
                elif k == FEED_CONFIG_AFTER:
                    _in_flight(ctx, f"run {k}")
                    ctx.wide_config(S, R, f, TAPS)
                    # (both calls made with work in flight lie behind: block 3, staged behind the reset, began from zeroed histories and carries)
                    _check_words(ctx.download_f32(), ys[k], f"floats of block {k}, the first behind m17hip_demod_reset")
            else:
                if FEED_HOW[k] != "host":
                    _check_words(ctx.download_f32(), ys[k], f"floats of block {k}")
                _check_records(_frames_once(ctx), rows[k])
                if k == FEED_FULL_RESET_AFTER:
                    ctx.reset()
                elif k == FEED_CONFIG_AFTER:
                    ctx.wide_config(S, R, f, TAPS)
        _check_records(_frames_once(ctx), rows[-1])
        _check_words(ctx.download_f32(), ys[-1], "floats of the last block")
        _check_diag(ctx.diag(CN), diags, DIAG_STREAM)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: both families on one stream, across the two streams ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow_case(wide_cases):
    """A narrowband int16 IQ block per channel (the eight basebands FM-modulated, one per channel in turn), T0 + TINY samples, and its floats from a zero
    carry."""
    import torch
    p = ol.gen_params(seed=20261021, kind=-1, n_frames=(T0 + TINY) // 1920 - 7, lead_in=3072, total=T0 + TINY)
    bb = ol.generate_batch(p, 8, T0 + TINY, threads=THREADS)
    z8 = [iq.fm_modulate(bb[i], sigma=400.0, cfo=0.01, fmt=iq.IQ_I16, seed=i + 1) for i in range(8)]
    z = np.stack([z8[c % 8] for c in range(CN)])
    pin = torch.from_numpy(z).pin_memory()
    return z, pin


def test_a_narrowband_block_staged_behind_a_wideband_block_in_flight(wide_cases, narrow_case):
    """m17hip_upload_iq_async at once after run 0 (a wideband block, tuned on the main stream) was queued: the discriminator on the copy stream finds the
    tuner's last z as its carry."""
    b = wide_cases["i16"]
    z, pin = narrow_case
    e = np.stack(_pool(lambda c: iq.discriminate(z[c, :TINY], 1.0, b.ref.carry[c])[0], CN))
    zero = np.stack([iq.discriminate(z[c, :4], 1.0, None)[0] for c in range(CN)])
    assert (_u32(zero[:, 0]) != _u32(e[:, 0])).all()
    ctx = context(b.fmt)
    try:
        _produce(ctx, b, "upload_wide_device")
        ctx.run()
        _in_flight(ctx)
        ctx.upload_iq_async(pin.data_ptr(), CN, TINY, pitch=T0 + TINY, iq_format=iq.IQ_I16)
        ctx.run(channels=CN, samples=TINY)
        _check_words(ctx.download_f32(), e, "a narrowband block behind a wideband one")
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), b.runs.rec0)
        ctx.upload_wait()
    finally:
        ctx.close()


def test_a_wideband_block_staged_behind_a_narrowband_block_in_flight(wide_cases, narrow_case):
    """The reverse: run 0 reads a discriminated narrowband block, the wideband block staged at once behind it takes each channel's first output against the
    narrowband block's last sample (the carry the discriminator left on the main stream), from fresh sources."""
    b = wide_cases["i16"]
    z, pin = narrow_case
    y0 = np.stack(_pool(lambda c: iq.discriminate(z[c, :T0], 1.0, None)[0], CN))
    ref = PFeeds(b.x, TAPS, SRC, FCW, R, GAIN)
    ref.carry = [z[c, T0 - 1].astype(np.float32) for c in range(CN)]
    e = ref.block(0, TINY)
    plain = PFeeds(b.x, TAPS, SRC, FCW, R, GAIN).block(0, 4)
    assert (_u32(plain[:, 0]) != _u32(e[:, 0])).all() and np.array_equal(_u32(plain[:, 1:]), _u32(e[:, 1:4]))
    r0, n0, _ = par._demod(y0, T0)
    ctx = context(b.fmt)
    try:
        ctx.upload_iq(np.ascontiguousarray(z[:, :T0]))
        ctx.run()
        _in_flight(ctx)
        ctx.upload_wide_device_async(b.dev.data_ptr(), CN, TINY, b.pitch, GAIN)
        ctx.run(channels=CN, samples=TINY)
        _check_words(ctx.download_f32(), e, "a wideband block behind a narrowband one")
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), par._flat(r0, np.zeros_like(n0), n0))
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 6: m17hip_set_stream with a run in flight -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["torch_stream", "null_stream"])
@pytest.mark.parametrize("staged", [False, True], ids=["in_place", "staged"])
@pytest.mark.parametrize("kind", ["wide_i16", "wide_u8"])
def test_set_stream_then_the_next_run(wide_cases, kind, staged, target):
    """The parent's case with a wideband kind: m17hip_set_stream at once after run 0 was queued, then the next block and run 1 on the new stream — the
    tuner's carries, histories and table follow the run there.  `staged`: tuning key 16, the in-place producers tune into the staging slab on the copy
    stream; or not (the tuner runs on the main stream and moves with it, behind the event the launch on the old stream left)."""
    import torch
    b = wide_cases[kind[5:]]
    r = b.runs
    side = torch.cuda.Stream() if target == "torch_stream" else None
    ctx = context(b.fmt)
    try:
        if staged:
            ctx.tune(16, 1)
        ctx.upload_wide(b.x0, gain=GAIN)
        ctx.run()
        _in_flight(ctx)
        ctx.set_stream(side.cuda_stream if side is not None else 0)
        assert ctx.stream == (side.cuda_stream if side is not None else 0)
        ctx.upload_wide(b.x1["full"], gain=GAIN)
        ctx.run()
        _check_records(_frames_once(ctx), r.rec1["full"])
        _check_diag(ctx.diag(CN), r.diag1["full"], DIAG_STREAM)
        _check_words(ctx.download_f32(), _words(b, "full"), "the floats run 1 read")
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), r.rec0)
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---- 7: a channel reset, then a staged block, with run 0 in flight -----------------------------------------------------------------------------------
# (in the live feed the block staged behind m17hip_demod_reset_channels is the one whose floats and records the feed gives up to the m17hip_demod_reset
# that follows: this is the case in which a tuner that did not wait for the carries' memset on the other stream shows)
@pytest.fixture(scope="module")
def reset_case(wide_cases):
    b = wide_cases["i16"]
    ref = copy.deepcopy(b.ref)
    for c in FEED_AGAIN:
        ref.carry[c] = np.zeros(2, dtype=np.float32)
    e1 = ref.block(T0, T0 + T1)
    rest = np.delete(np.arange(CN), FEED_AGAIN)
    assert (e1[FEED_AGAIN, 0] == 0).all() and (b.y[FEED_AGAIN, T0] != 0).all() and np.array_equal(_u32(e1[rest]), _u32(b.y[rest, T0:]))
    assert np.array_equal(_u32(e1[:, 1:]), _u32(b.y[:, T0 + 1:])), "only the first output behind the reset differs: the history is the source's"
    origin = np.zeros(CN, dtype=np.int64)
    origin[FEED_AGAIN] = T0
    exp = Expect(np.concatenate([b.y[:, :T0], e1], axis=1), origin=origin)
    rows = exp.run(T0, T0 + T1)
    assert all(rows[c].size > 0 and rows[c]["seq"][0] == 0 for c in FEED_AGAIN if c in GROUPS["stream"]), "the listed stream channels' records restart"
    return e1, np.concatenate(rows)


@pytest.mark.parametrize("producer,stage", [("upload_wide", "async_full"), ("upload_wide_device", "device_async")])
def test_channel_reset_then_a_staged_block_with_run_0_in_flight(wide_cases, reset_case, producer, stage):
    """m17hip_demod_reset_channels at once after run 0 (its block tuned on the main stream) was queued: the listed carries are zeroed on the main stream,
    behind run 0.  The block staged at once behind the call is tuned on the copy stream and must find the zeroes: the listed channels' first output is +0,
    every other float is the unbroken feed's (the histories are the sources').  The block from pinned memory follows a host producer: behind a device
    producer it would be the context's first block through the raw buffer, whose allocation waits for the memset and with it for run 0 — the tuner then
    finds the zeroes whatever it waits for."""
    b = wide_cases["i16"]
    e1, rec1 = reset_case
    ctx = context(b.fmt)
    try:
        _produce(ctx, b, producer)
        ctx.run()
        _in_flight(ctx)
        ctx.reset_channels(FEED_AGAIN)
        _stage(ctx, b, stage)
        ctx.run(channels=CN, samples=T1)
        _check_words(ctx.download_f32(), e1, "the floats of the block staged behind the reset")
        _check_records(_frames_once(ctx), rec1)
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), b.runs.rec0)
        ctx.upload_wait()
    finally:
        ctx.close()
