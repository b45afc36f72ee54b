"""GPU tests of the host-side call orders of the float (ABI 607), IQ (ABI 608) and voice (ABI 606) paths with a run STILL IN FLIGHT: the regime of
tests/test_gpu_call_orders.py (queue a run that stays on the device for milliseconds, make the call under test at once, compare with the oracle byte for
byte) for the cross-stream paths those three features added — the float slab pair zeroed on the stream that writes it and the float tail carried across
runs, the discriminator's carry and the raw-IQ buffer ordered by one event between the main and the copy stream, the voice consumer's per-channel state
carried on a payload stream that changes at the first staging.  Every case has a FRESH context: the stream change under test is its first.

Shape: 64 channels, run 0 = 96 000 samples, run 1 = one 1920-sample frame ("tiny") or the next 24 000 samples ("full") of every channel.  How long
a run stays on the device is set by the per-channel sequential chains, so by its length in samples and not by the channel count, while the oracle's cost
grows with the channels: few channels, long rows.  Measured once on the MI355X (a throwaway context and staging first; six fresh contexts per input kind;
from the return of m17hip_demod_run to the end of its work on the main stream; the host-side duration of every first staging the cases use, three fresh
contexts each, float and IQ in both layouts, host and device producers):
    run 0 at 64 x  96 000:  3.66 - 3.80 ms in flight   longest staging 0.27 ms   ratio 13.7
    run 0 at 64 x 192 000:  5.17 - 6.50 ms             longest staging 0.30 ms   ratio 17.1
    run 0 at 64 x 480 000: 10.17 - 10.89 ms            longest staging 0.31 ms   ratio 32.8
The smallest length whose shortest in-flight time is at least four times the longest staging time is taken: 96 000 (the int16 file lives with a margin of
about three).  The slowest stagings are tuning key 16 with an in-place upload (0.12 - 0.27 ms: it waits for its own copy) and the first float staging from
pinned memory of a context whose producer read device memory (0.27 ms once, 0.06 ms after).  Beyond the margin every case asserts its own premise: just
before the call under test the context's main stream is asked, without waiting, whether it has work outstanding (_in_flight) — the last kernels of a run's
chain (the carried tails, settle_tail_kernel) and the events the fetches wait for are queued on that stream (end_run in csrc/m17hip.hip) — and a case whose
run 0 had already finished FAILS.
Durations on the MI355X: a case 0.01 - 0.03 s; the four module fixtures (the oracles, 16 threads) 0.3 - 0.9 s each; the 128 tests of the module under 5 s.
"""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import voice_log as vl

pytestmark = pytest.mark.gpu

CN, T0, TINY = 64, 96000, 1920
T1 = T0 // 4
THREADS = 16
assert T0 % 192 == 0 and T1 % 192 == 0

# the diagnostics of ONE run from a reset and those of a continued stream: the field lists of tests/test_gpu_call_orders.py
DIAG_EXACT = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
DIAG_FLOAT = ("evm", "deviation", "offset", "clock", "dcd_level")
DIAG_STREAM = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "evm", "deviation", "offset", "clock")

FMTS = {"i16": iq.IQ_I16, "f32": iq.IQ_F32}
SAMPLE_BYTES = {iq.IQ_I16: 4, iq.IQ_F32: 8}
AFTERS = ("direct", "front", "run_select1")
STAGES = ("async_tiny", "async_full", "device_async", "tune16_upload")
CHUNK = {"async_tiny": "tiny", "async_full": "full", "device_async": "full", "tune16_upload": "tiny"}
LEN = {"tiny": TINY, "full": T1}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _flat(recs, lo, hi):
    return np.concatenate([recs[c, lo[c]: hi[c]] for c in range(recs.shape[0])])


def _rec_cap(T):
    return 2 * (T // 1920 + 2) + 4


def _demod(x, T):
    """The oracle of x's sample type over the first T samples of every row: (recs[C][cap], counts[C], diags[C])."""
    head = np.ascontiguousarray(x[:, :T])
    if head.dtype == np.float32:
        return fl.demod_batch(head, threads=THREADS)
    return ol.demod_batch(head, cap=_rec_cap(T), threads=THREADS)


def baseband(seed=20261018):
    """BERT (even) and stream (odd) channels as the generator mixes them (kind -1), T0 + T0 / 4 samples, noise sigma 600, loud lead-in."""
    total = T0 + T1
    p = ol.gen_params(seed=seed, kind=-1, n_frames=total // 1920 - 7, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0, total=total)
    return ol.generate_batch(p, CN, total, threads=THREADS)


class Runs:
    """The oracle's view of CN rows of T0 + T1 samples (int16, or floats in the reference's units): run 0 = the first T0 samples, run 1 = the next T1
    ("full") or TINY ("tiny") of every channel.  The demodulator is causal: run 0's records are the first records of the longer streams (asserted)."""

    def __init__(self, x):
        r0, n0, self.diag0 = _demod(x, T0)
        self.n0 = n0
        self.rows0 = [r0[c, : n0[c]] for c in range(CN)]
        self.rec0 = _flat(r0, np.zeros_like(n0), n0)
        self.rec1, self.diag1, self.rows1 = {}, {}, {}
        for name, t in LEN.items():
            r, n, d = _demod(x, T0 + t)
            assert all(r[c, : n0[c]].tobytes() == r0[c, : n0[c]].tobytes() for c in range(CN)), f"run 0's records are no prefix of the {name} stream's"
            self.rec1[name], self.diag1[name] = _flat(r, n0, n), d
            self.rows1[name] = [r[c, n0[c]: n[c]] for c in range(CN)]

    def assert_records_in_both_runs(self, groups):
        """Every channel group the cases rely on yields records in run 0 and in the full run 1 (and the one frame of the tiny run 1 some at all)."""
        for name, chans in groups.items():
            assert all(self.rows0[c].size > 0 for c in chans), f"{name}: a channel without records in run 0"
            assert all(self.rows1["full"][c].size > 0 for c in chans), f"{name}: a channel without records in run 1"
        assert self.rec1["tiny"].size > 0


GROUPS = {"bert": range(0, CN, 2), "stream": range(1, CN, 2)}


def float_stream():
    """Floats off the int16 grid (another gain, a DC offset, no quantisation): a float path that secretly rounded would differ."""
    x = fl.off_grid(baseband(), seed=607)
    assert fl.survives_round_trip(x).mean() < 0.01
    runs = Runs(x)
    runs.assert_records_in_both_runs(GROUPS)
    return x, runs


def iq_stream(fmt):
    """The baseband FM-modulated (sigma 400 per component, 0.01 rad per sample off frequency) in one layout; the expected floats are the host form's over
    the WHOLE row — the first float of run 1's block depends on the carry run 0's block left — and the expected records the float oracle's on those."""
    s = baseband()
    z = np.stack([iq.fm_modulate(s[c], sigma=400.0, cfo=0.01, fmt=fmt, seed=c + 1) for c in range(CN)])
    y = iq.discriminate_rows(z, 1.0)[0]
    assert np.isfinite(y).all()
    fresh = np.stack([iq.discriminate(z[c, T0:T0 + 4], 1.0, None)[0] for c in range(CN)])
    assert (_u32(fresh[:, 0]) != _u32(y[:, T0])).all(), "the first float of run 1's block is the one the carry decides"
    runs = Runs(y)
    runs.assert_records_in_both_runs(GROUPS)
    return z, y, runs


# ---- voice: stream transmissions whose lengths are drawn per channel -----------------------------------------------------------------------
VOICE_SEED = 2
VOICE_ROOM = (T0 + T1) // 1920 + 8     # stream records per channel and run the planes hold (tuning key 34)


def voice_baseband(seed):
    """Per channel up to two stream transmissions (kind 1) back to back: A closes inside run 0; B sends its LSF inside run 0 and its last frame inside the
    full run 1.  Which of the two a channel has, their lengths and where B begins (off the frame grid) are drawn per channel."""
    rng = np.random.default_rng(seed)
    total, F0, F1 = T0 + T1, T0 // 1920, T1 // 1920
    s = np.zeros((CN, total), dtype=np.int16)

    def part(kind, n_frames, n):
        p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=kind, n_frames=n_frames, lead_in=3072, lead_sigma=40000.0, noise_sigma=600.0,
                          tail_sigma=600.0, total=n)
        return ol.generate(p)[:n]

    for c in range(CN):
        has_a = rng.random() < 0.75
        has_b = rng.random() < 0.6 or not has_a
        k = int(rng.integers(4, min(16, F0 // 3) + 1))                       # B's preamble begins k frames (and a jitter) before the end of run 0
        cut = T0 - k * 1920 - int(rng.integers(0, 1920)) - 3072
        n_b = k + int(rng.integers(2, F1 - 5))                               # ... and its last frame ends 2 .. F1 - 4 frames into run 1
        n_a = int(rng.integers(3, (cut - 3072 - 3000) // 1920 - 3))
        s[c, :cut] = part(1 if has_a else 3, n_a, cut)
        s[c, cut:] = part(1 if has_b else 3, n_b, total - cut)
    return s


class VoiceRuns(Runs):
    """Runs, and what the restated voice consumer (tests/voice_log.py) makes of their records run by run, its state carried from run 0 into run 1."""

    def __init__(self, x):
        super().__init__(x)
        bank = vl.VoiceBank(CN)
        self.v0 = bank.feed(self.rows0, slots=1)
        self.open0 = [None if log.call is None else dict(log.call) for log in bank.logs]
        self.v1 = {name: copy.deepcopy(bank).feed(self.rows1[name], slots=1) for name in LEN}
        # what makes the cases bite, on the oracle's records alone
        calls0, calls1 = self.v0[3], self.v1["full"][3]
        closers = set(int(ch) for ch in calls0["channel"])
        assert len(closers) >= CN // 2, f"{len(closers)} channels close a call inside run 0"
        self.spanning = []
        for c in range(CN):
            mine = calls1[calls1["channel"] == c]
            o = self.open0[c]
            if o is not None and o["has_lsf"] and o["frames"] >= 1 and mine.size and int(mine[0]["start_pos"]) == o["start_pos"] < T0 <= int(mine[0]["end_pos"]):
                assert bytes(mine[0]["lsf"]) == o["lsf"] and int(mine[0]["frames"]) > o["frames"] and int(mine[0]["seq"]) == (calls0["channel"] == c).sum()
                self.spanning.append(c)
        assert len(self.spanning) >= CN // 4, f"{len(self.spanning)} channels carry an open call (LSF captured in run 0) into run 1 and close it there"
        assert all(self.rows0[c].size and self.rows1["full"][c].size for c in self.spanning)
        assert max(int(self.v0[2].max()), int(self.v1["full"][2].max())) <= VOICE_ROOM

    def after_reset(self, x, again):
        """Run 1 (full) with the channels `again` started over at T0: their records are a fresh demodulator's over x[c, T0:], their call log is a fresh
        consumer's — the call they had open is abandoned, never reported."""
        sub = np.ascontiguousarray(x[again, T0:])
        r, n, _ = _demod(sub, T1)
        rows = list(self.rows1["full"])
        bank = vl.VoiceBank(CN)
        bank.feed(self.rows0)
        for i, c in enumerate(again):
            rows[c] = r[i, : n[i]].copy()
            rows[c]["channel"] = c
            bank.logs[c].reset()
        v1 = bank.feed(rows, slots=1)
        # one hand-made LSF record per channel (m17hip_voice_feed) closes whatever a channel still has open: an abandoned call would show here
        closing = np.zeros((CN, 1), dtype=m17hip.FRAME_REC)
        for c in range(CN):
            closing[c, 0]["channel"], closing[c, 0]["sample_pos"], closing[c, 0]["len"] = c, 10 ** 6 + c, 30
            closing[c, 0]["payload"][:30] = c
        quiet = [c for c in again if bank.logs[c].call is None]
        assert len(quiet) >= max(1, len(again) // 2), "restarted inside a transmission, most of the listed channels open no call of their own in run 1"
        vc = bank.feed([closing[c] for c in range(CN)], slots=1)
        assert not np.isin(vc[3]["channel"], quiet).any() and vc[3].size >= CN // 8
        return np.concatenate(rows), v1, closing, vc


def voice_streams(seed=VOICE_SEED):
    s = voice_baseband(seed)
    x = fl.off_grid(s, seed=606)
    return {"i16": (s, VoiceRuns(s)), "f32": (x, VoiceRuns(x))}


# ---- a live IQ feed ----------------------------------------------------------------------------------------------------------------------------
# six blocks of T0 / 4; blocks 1 and 3 (host memory: they go through the raw-IQ buffer) are longer than all before them, so the buffer grows while the
# block before may still be read
FEED_LEN = (T1, T1 + 1920, T1, T1 + 3840, T1, T1)
FEED_HOW = ("pinned", "host", "device", "pinned", "host", "device")
FEED_CUTS = np.concatenate([[0], np.cumsum(FEED_LEN)]).tolist()
FEED_RESET_AFTER = 1                        # m17hip_demod_reset_channels at once after this run was queued
FEED_AGAIN = np.arange(1, CN, 3)            # a third of the channels


class Expect:
    """The float oracle over whole streams y[C][T] (channel c from sample origin[c] on): the records of the run that covers samples [b0, b1) of the
    context's stream (tests/test_gpu_iq_input.py's Expect, without the diagnostic log)."""

    def __init__(self, y, origin=None):
        self.C, self.T = y.shape
        self.origin = np.zeros(self.C, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
        self.recs, self.diags = [None] * self.C, np.zeros(self.C, dtype=ol.DIAG)
        for a in np.unique(self.origin):
            chs = np.flatnonzero(self.origin == a)
            r, n, d = fl.demod_batch(np.ascontiguousarray(y[chs, a:]), threads=THREADS)
            for i, c in enumerate(chs):
                self.recs[c] = r[i, : n[i]].copy()
                self.recs[c]["channel"] = c
                self.diags[c] = d[i]

    def run(self, b0, b1):
        rows = []
        for c in range(self.C):
            lo, hi = b0 - self.origin[c], b1 - self.origin[c]
            r = self.recs[c]
            rows.append(r[(r["sample_pos"] >= max(lo, 0)) & (r["sample_pos"] < hi)].copy())
        return rows


def feed_case(fmt, seed=20261019):
    total = FEED_CUTS[-1]
    p = ol.gen_params(seed=seed, kind=-1, n_frames=total // 1920 - 7, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0, total=total)
    s = ol.generate_batch(p, CN, total, threads=THREADS)
    z = np.stack([iq.fm_modulate(s[c], sigma=400.0, cfo=0.01, fmt=fmt, seed=c + 1) for c in range(CN)])
    y = iq.discriminate_rows(z, 1.0)[0]
    at = FEED_CUTS[FEED_RESET_AFTER + 1]
    assert at % 192 == 0
    origin = np.zeros(CN, dtype=np.int64)
    origin[FEED_AGAIN] = at
    for c in FEED_AGAIN:   # (a feed that starts over: from a zero carry, the first float is +0)
        head = y[c, at]
        y[c, at:] = iq.discriminate(z[c, at:], 1.0, None)[0]
        assert _u32(y[c, at]) == 0 and head != 0
    exp = Expect(y, origin=origin)
    first = Expect(np.ascontiguousarray(y[FEED_AGAIN, :at]))   # (before they start over, the channels concerned are channels like any other)
    rows = []
    for k in range(len(FEED_LEN)):
        r = exp.run(FEED_CUTS[k], FEED_CUTS[k + 1])
        if k <= FEED_RESET_AFTER:
            f = first.run(FEED_CUTS[k], FEED_CUTS[k + 1])
            for i, c in enumerate(FEED_AGAIN):
                r[c] = f[i]
                r[c]["channel"] = c
        assert sum(q.size for q in r) > CN, f"run {k} yields records"
        rows.append(np.concatenate(r))
    after = exp.run(at, total)
    assert all(after[c].size > 4 and after[c]["seq"][0] == 0 for c in FEED_AGAIN), "the listed channels' records restart"
    return z, y, rows, exp.diags


# ---- fixtures: the expectation once on the CPU, then what the producers and stagings read ------------------------------------------------
class Buffers:
    """x[CN][T0 + T1] (float32, int16, complex64 or int16 pairs) as run 0's block and the two chunks after it: in host memory, pinned, on the device."""

    def __init__(self, x, runs, y=None):
        import torch
        self.x, self.runs, self.y = x, runs, y
        self.x0 = np.ascontiguousarray(x[:, :T0])
        self.x1 = {"full": np.ascontiguousarray(x[:, T0:]), "tiny": np.ascontiguousarray(x[:, T0:T0 + TINY])}
        self.pin1 = {k: torch.from_numpy(v).pin_memory() for k, v in self.x1.items()}
        self.dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.sample_bytes = x[0, 0].nbytes
        self.recbuf = torch.empty(CN * _rec_cap(T0 + T1) * m17hip.FRAME_REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                         # (the producers' buffers are complete before they are handed over: include/m17hip.h)
        self.dev1 = self.dev.data_ptr() + self.sample_bytes * T0


@pytest.fixture(scope="module", autouse=True)
def first_staging_of_the_process():
    """One throwaway context and staging before any case: the first staging of a process costs about 15 ms in allocations (the copy stream, the pools),
    several times what run 0 stays in flight — the first case of the module would find run 0 finished (it did, and failed its premise)."""
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


@pytest.fixture(scope="module")
def f32_case():
    return Buffers(*float_stream())


@pytest.fixture(scope="module")
def iq_cases():
    out = {}
    for name, f in FMTS.items():
        z, y, runs = iq_stream(f)
        out[name] = Buffers(z, runs, y)
        out[name].fmt = f
    return out


@pytest.fixture(scope="module")
def voice_cases():
    """Generator seed VOICE_SEED: the first for which the premises of VoiceRuns hold for the int16 and for the float stream (searched on the CPU)."""
    return {name: Buffers(x, runs) for name, (x, runs) in voice_streams().items()}


@pytest.fixture(scope="module")
def feed_cases():
    import torch
    out = {}
    for name, f in FMTS.items():
        z, y, rows, diags = feed_case(f)
        pin, dev = torch.from_numpy(z).pin_memory(), torch.from_numpy(z).cuda()
        torch.cuda.synchronize()
        out[name] = (z, y, rows, diags, pin, dev)
    return out


# ---- the steps of a case ---------------------------------------------------------------------------------------------------------------------
def _in_flight(ctx, what="run 0"):
    """The premise of every case: the main stream (the last kernels of a run's chain — the carried tails, settle_tail_kernel — are queued on it, and so
    are the events the fetch family waits for) still has work outstanding when the call under test is made.  Asked without waiting."""
    import torch
    assert not torch.cuda.ExternalStream(ctx.stream).query(), \
        f"{what} had already finished on the device before the call under test was made: this case cannot show an ordering error (not a pass)"


def _frames_once(ctx):
    """m17hip_frames_fetch ONCE with room for every record (Context.frames repeats a fetch that was too small, and a repeat comes late)."""
    recs = np.zeros(CN * _rec_cap(T0 + T1), dtype=m17hip.FRAME_REC)
    got = C.c_uint64(0)
    ctx._chk(ctx.lib.m17hip_frames_fetch(ctx.h, m17hip._ptr(recs), C.c_uint64(recs.size), C.byref(got)))
    return recs[: got.value]


def _compact_device(ctx, b):
    n = ctx.frames_compact_device(b.recbuf.data_ptr(), CN * _rec_cap(T0 + T1))
    return b.recbuf[: n * m17hip.FRAME_REC.itemsize].cpu().numpy().view(m17hip.FRAME_REC)


def _check_diag(d, exp, fields):
    for f in fields:
        assert np.array_equal(d[f], exp[f], equal_nan=True), (f, np.flatnonzero(d[f] != exp[f])[:16].tolist())


def _check_records(got, exp):
    assert got.size == exp.size, (got.size, exp.size)
    assert got.tobytes() == exp.tobytes()


def _check_words(got, exp, what):
    bad = np.argwhere(_u32(got) != _u32(exp))
    assert got.shape == exp.shape and bad.size == 0, (what, bad.shape[0], bad[:8].tolist())


def _produce(ctx, b, producer):
    """Run 0's input, written in place."""
    if producer == "upload":
        ctx.upload(b.x0)
    elif producer == "upload_device":
        ctx.upload_device(b.dev.data_ptr(), CN, T0, pitch=T0 + T1, dtype=b.x.dtype)
    elif producer == "upload_iq":
        ctx.upload_iq(b.x0)
    else:
        ctx.upload_iq_device(b.dev.data_ptr(), CN, T0, pitch=T0 + T1, iq_format=b.fmt)


def _stage(ctx, b, stage):
    """The context's first staged input: the chunk after run 0, in the format of the stream."""
    chunk = CHUNK[stage]
    t = LEN[chunk]
    if b.y is not None:                                  # an IQ stream
        if stage in ("async_tiny", "async_full"):
            ctx.upload_iq_async(b.pin1[chunk].data_ptr(), CN, t, iq_format=b.fmt)
        elif stage == "device_async":
            ctx.upload_iq_device_async(b.dev1, CN, t, pitch=T0 + T1, iq_format=b.fmt)
        else:
            ctx.tune(16, 1)
            ctx.upload_iq(b.x1[chunk])
    elif stage in ("async_tiny", "async_full"):
        ctx.upload_async(b.pin1[chunk].data_ptr(), CN, t, dtype=b.x.dtype)
    elif stage == "device_async":
        ctx.upload_device_async(b.dev1, CN, t, pitch=T0 + T1, dtype=b.x.dtype)
    else:
        ctx.tune(16, 1)
        ctx.upload(b.x1[chunk])


def _then(ctx, after, t):
    if after == "front":
        ctx.front(channels=CN, samples=t)
    elif after == "run_select1":
        ctx.run(channels=CN, samples=t)
        ctx.frames_select(1)


def _call(ctx, b, call, after, chunk):
    """The call under test, checked against what the run it names (the selected run; m17_diag: the latest) holds."""
    r = b.runs
    latest_diag, latest_fields = (r.diag1[chunk], DIAG_STREAM) if after == "run_select1" else (r.diag0, DIAG_EXACT + DIAG_FLOAT)
    _in_flight(ctx)
    if call == "frames_count":
        assert ctx.frames_count() == r.rec0.size
    elif call == "frames":
        _check_records(_frames_once(ctx), r.rec0)
    elif call == "compact_device":
        _check_records(_compact_device(ctx, b), r.rec0)
    else:
        _check_diag(ctx.diag(CN), latest_diag, latest_fields)


def _input_words(b, chunk):
    """The floats run 1 reads: the uploaded chunk itself, or (IQ) the host form's floats of that block."""
    src = b.x if b.y is None else b.y
    return src[:, T0:T0 + LEN[chunk]]


def _case(b, producer, stage, call, after):
    ctx = m17hip.Context(CN, T0)
    try:
        chunk = CHUNK[stage]
        t = LEN[chunk]
        _produce(ctx, b, producer)
        ctx.run()
        _stage(ctx, b, stage)                            # run 0 is still on the device: nothing in between synchronises
        _then(ctx, after, t)
        _call(ctx, b, call, after, chunk)
        # the stream goes on: run 1 on the staged chunk, then every fetch once more
        if after != "run_select1":
            ctx.run(channels=CN, samples=t)
        r = b.runs
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), r.rec0)
        ctx.frames_select(0)
        assert ctx.frames_count() == r.rec1[chunk].size
        _check_records(_frames_once(ctx), r.rec1[chunk])
        _check_records(_compact_device(ctx, b), r.rec1[chunk])
        _check_diag(ctx.diag(CN), r.diag1[chunk], DIAG_STREAM)
        _check_words(ctx.download_f32(), _input_words(b, chunk), "the floats run 1 read")
        ctx.upload_wait()
    finally:
        ctx.close()


def _matrix(calls, producers, fmts=(None,)):
    """Every (call, what follows the staging) pair twice, with two different stagings; the producer and the staging rotate so that every
    (producer, staging) pair is met — per format where there are two."""
    out = []
    for fmt in fmts:
        for shift in (0, 1):   # (two producers over four stagings: an even shift would only ever pair producer i with the stagings i, i + 2)
            for i, (call, after) in enumerate(itertools.product(calls, AFTERS)):
                producer, stage = producers[i % len(producers)], STAGES[(i + shift) % len(STAGES)]
                args = (producer, stage, call, after) if fmt is None else (fmt, producer, stage, call, after)
                out.append(pytest.param(*args, id="-".join(args)))
    return out


FETCHES = ("frames_count", "frames", "compact_device", "diag")


def test_the_matrices_meet_every_producer_and_staging():
    """(No GPU work.)  The rotation reaches every (producer, staging) pair, per format."""
    for producers, fmts in ((("upload", "upload_device"), (None,)), (("upload_iq", "upload_iq_device"), tuple(FMTS))):
        for fmt in fmts:
            seen = set(p.values[-4:-2] for p in _matrix(FETCHES, producers, fmts) if fmt is None or p.values[0] == fmt)
            assert seen == set(itertools.product(producers, STAGES))
    seen = set(p.values[1:3] for p in _matrix(VOICE_CALLS, ("upload", "upload_device"), ("i16", "f32")))
    assert seen == set(itertools.product(("upload", "upload_device"), STAGES))


# ---- 1: float input ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("producer,stage,call,after", _matrix(FETCHES, ("upload", "upload_device")))
def test_float_fetch_right_after_the_first_staging(f32_case, producer, stage, call, after):
    """A float stream: run 0 in place, the first float staging at once (it allocates the second float slab and zeroes its prefix on the copy stream), then
    (directly, behind a front end of run 1, or behind run 1 with run 0 selected) a fetch: it names run 0 and must wait for it.  Run 1 continues the stream
    from the float tail run 0 carried; its input is read back byte for byte."""
    _case(f32_case, producer, stage, call, after)


def test_float_in_place_upload_with_run_0_in_flight(f32_case):
    """No staging at all: a float context's first in-place upload of run 1 (`inplace_after_run`) is made while run 0 still reads the slab it overwrites."""
    b, r = f32_case, f32_case.runs
    ctx = m17hip.Context(CN, T0)
    try:
        ctx.upload(b.x0)
        ctx.run()
        _in_flight(ctx)
        ctx.upload(b.x1["full"])
        _check_words(ctx.download_f32(), b.x1["full"], "the floats run 1 reads")
        ctx.run()
        _check_records(_frames_once(ctx), r.rec1["full"])
        _check_diag(ctx.diag(CN), r.diag1["full"], DIAG_STREAM)
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), r.rec0)
    finally:
        ctx.close()


# ---- 2: IQ input, both layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,producer,stage,call,after", _matrix(FETCHES, ("upload_iq", "upload_iq_device"), tuple(FMTS)))
def test_iq_fetch_right_after_the_first_staging(iq_cases, fmt, producer, stage, call, after):
    """An IQ stream: run 0's block discriminated in place on the main stream, the next block staged at once — its discriminator runs on the copy stream,
    behind the carry (and, from host memory, the raw-IQ buffer) the main stream's launch left — then the fetch.  After run 1 the discriminated floats of
    its block are compared as words with the host form over the whole row: the first column is the one the carry decides."""
    _case(iq_cases[fmt], producer, stage, call, after)


# ---- 3: a live IQ feed at this size ----------------------------------------------------------------------------------------------------------
def _feed_block(ctx, z, pin, dev, f, k):
    a, n, sb = FEED_CUTS[k], FEED_LEN[k], SAMPLE_BYTES[f]
    if FEED_HOW[k] == "pinned":
        ctx.upload_iq_async(pin.data_ptr() + a * sb, CN, n, pitch=FEED_CUTS[-1], iq_format=f)
    elif FEED_HOW[k] == "host":
        ctx.upload_iq(z[:, a:a + n])
    else:
        ctx.upload_iq_device_async(dev.data_ptr() + a * sb, CN, n, pitch=FEED_CUTS[-1], iq_format=f)


@pytest.mark.parametrize("check", ["records_behind_the_next_run", "floats_and_records_run_by_run"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_live_iq_feed(feed_cases, fmt, check):
    """Six blocks — staged from pinned host memory, in place from host memory (the raw buffer is written from the other stream than the one before),
    staged from device memory, and again — with no host synchronisation beyond what the calls themselves do; the raw-IQ buffer grows twice while the block
    before may still be read; a third of the channels start over (m17hip_demod_reset_channels) at once after run 1 was queued: their next block begins
    from a zero carry on the OTHER stream, their records restart.  `records_behind_the_next_run`: run k's records are fetched behind run k + 1
    (m17hip_frames_select) and only the in-place blocks' floats are read back, so the device never drains; the other order reads every block's floats."""
    z, y, rows, diags, pin, dev = feed_cases[fmt]
    f = FMTS[fmt]
    live = check == "records_behind_the_next_run"
    ctx = m17hip.Context(CN, max(FEED_LEN))
    try:
        for k, n in enumerate(FEED_LEN):
            _feed_block(ctx, z, pin, dev, f, k)
            block = y[:, FEED_CUTS[k]:FEED_CUTS[k + 1]]
            if FEED_HOW[k] == "host":
                _check_words(ctx.download_f32(), block, f"floats of block {k}")
            ctx.run(channels=CN, samples=n)
            if k == FEED_RESET_AFTER:
                _in_flight(ctx, f"run {k}")
                ctx.reset_channels(FEED_AGAIN)
            if live:
                if k > 0:
                    ctx.frames_select(1)
                    _check_records(_frames_once(ctx), rows[k - 1])
                    ctx.frames_select(0)
            else:
                if FEED_HOW[k] != "host":
                    _check_words(ctx.download_f32(), block, f"floats of block {k}")
                _check_records(_frames_once(ctx), rows[k])
        _check_records(_frames_once(ctx), rows[-1])
        _check_words(ctx.download_f32(), y[:, FEED_CUTS[-2]:], "floats of the last block")
        _check_diag(ctx.diag(CN), diags, DIAG_STREAM)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4: the voice consumer (tuning key 34 before run 0) ------------------------------------------------------------------------------------
VOICE_CALLS = ("voice", "calls", "voice_device")
CALL_CAP = CN * m17hip.calls_per_channel(VOICE_ROOM)


def _voice_once(ctx):
    """m17hip_voice_fetch ONCE, the planes as wide as the room (Context.voice asks for the counts first: a second call comes late)."""
    audio = np.zeros((CN, VOICE_ROOM, 16), dtype=np.uint8)
    marks = np.zeros((CN, VOICE_ROOM), dtype=np.uint8)
    counts = np.zeros(CN, dtype=np.uint32)
    ctx._chk(ctx.lib.m17hip_voice_fetch(ctx.h, m17hip._ptr(audio), m17hip._ptr(marks), m17hip._ptr(counts), C.c_uint32(CN), C.c_uint32(VOICE_ROOM)))
    return audio, marks, counts


def _voice_device(ctx):
    """The planes where they lie, through the pointers m17hip_voice_device returns."""
    import torch
    a_dev, m_dev, n_dev, pitch = ctx.voice_device()
    assert a_dev and m_dev and n_dev and pitch == VOICE_ROOM
    view = lambda ptr, shape, typestr: torch.as_tensor(type("DeviceView", (), {"__cuda_array_interface__": dict(
        shape=shape, typestr=typestr, data=(ptr, False), version=2)})(), device="cuda")
    counts = view(n_dev, (CN,), "<i4").cpu().numpy().astype(np.uint32)
    return view(a_dev, (CN, pitch, 16), "|u1").cpu().numpy(), view(m_dev, (CN, pitch), "|u1").cpu().numpy(), counts


def _check_planes(got, exp, what):
    assert np.array_equal(got[2], exp[2]), (what, "counts", np.flatnonzero(got[2] != exp[2])[:16].tolist())
    for c, n in enumerate(exp[2]):
        assert got[1][c, :n].tobytes() == exp[1][c, :n].tobytes(), (what, "marks", c)
        assert got[0][c, :n].tobytes() == exp[0][c, :n].tobytes(), (what, "audio", c)


def _check_calls(got, exp, what):
    assert got.size == exp.size, (what, got.size, exp.size)
    assert got.tobytes() == exp.tobytes(), (what, [i for i in range(exp.size) if got[i] != exp[i]][:4])


def _voice_call(ctx, v, call, what):
    if call == "voice":
        _check_planes(_voice_once(ctx), v, what)
    elif call == "calls":
        _check_calls(ctx.calls(capacity=CALL_CAP), v[3], what)
    else:
        _check_planes(_voice_device(ctx), v, what)


@pytest.mark.parametrize("fmt,producer,stage,call,after", _matrix(VOICE_CALLS, ("upload", "upload_device"), ("i16", "f32")))
def test_voice_fetch_right_after_the_first_staging(voice_cases, fmt, producer, stage, call, after):
    """The voice consumer of run 0 was queued on the main stream; the first staging makes the copy stream the payload stream, and the fetch (planes, calls,
    device pointers — of run 0, also behind run 1 with run 0 selected) is queued there.  Run 1's consumer then continues every open call from the state run
    0's consumer left on the other stream: a call that spans the runs is reported once, by run 1, with run 0's LSF and start position and both runs' totals."""
    b = voice_cases[fmt]
    r = b.runs
    ctx = m17hip.Context(CN, T0)
    try:
        ctx.tune(34, VOICE_ROOM)
        chunk = CHUNK[stage]
        t = LEN[chunk]
        _produce(ctx, b, producer)
        ctx.run()
        _stage(ctx, b, stage)
        _then(ctx, after, t)
        _in_flight(ctx)
        _voice_call(ctx, r.v0, call, "run 0, the call under test")
        if after != "run_select1":
            ctx.run(channels=CN, samples=t)
        ctx.frames_select(1)
        for c in VOICE_CALLS:
            _voice_call(ctx, r.v0, c, f"run 0 once more, {c}")
        _check_records(_frames_once(ctx), r.rec0)
        ctx.frames_select(0)
        for c in VOICE_CALLS:
            _voice_call(ctx, r.v1[chunk], c, f"run 1, {c}")
        _check_records(_frames_once(ctx), r.rec1[chunk])
        if chunk == "full":                              # (stated once more in the open: what the byte comparison above has already shown)
            got = ctx.calls(capacity=CALL_CAP)
            for c in r.spanning:
                q = got[got["channel"] == c][0]
                o = r.open0[c]
                assert int(q["start_pos"]) == o["start_pos"] < T0 and bytes(q["lsf"]) == o["lsf"] and q["has_lsf"] == 1 and int(q["frames"]) > o["frames"]
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["i16", "f32"])
def test_voice_channel_reset_with_run_0_in_flight(voice_cases, fmt):
    """m17hip_demod_reset_channels at once after run 0 was queued, for channels that have a call open at its end, then run 1 staged: the reset of the
    consumers' state is queued on the new payload stream and must come behind run 0's consumer on the old one.  The open call is abandoned (never
    reported, as tests/test_gpu_voice.py::test_a_channel_reset_abandons_its_open_call states it, also not when a hand-made LSF record per channel closes
    whatever is open at the end); the other channels' calls span the runs as before."""
    b = voice_cases[fmt]
    r = b.runs
    again = np.array(r.spanning[::2])
    rec1, v1, closing, vc = r.after_reset(b.x, again)
    assert again.size >= CN // 8
    ctx = m17hip.Context(CN, T0)
    try:
        ctx.tune(34, VOICE_ROOM)
        ctx.upload(b.x0)
        ctx.run()
        _in_flight(ctx)
        ctx.reset_channels(again)
        ctx.upload_async(b.pin1["full"].data_ptr(), CN, T1, dtype=b.x.dtype)
        ctx.run(channels=CN, samples=T1)
        ctx.frames_select(1)
        for c in VOICE_CALLS:
            _voice_call(ctx, r.v0, c, f"run 0, {c}")
        _check_records(_frames_once(ctx), r.rec0)
        ctx.frames_select(0)
        for c in VOICE_CALLS:
            _voice_call(ctx, v1, c, f"run 1, {c}")
        _check_records(_frames_once(ctx), rec1)
        ctx.upload_wait()
        ctx.voice_feed(closing, np.ones(CN, dtype=np.uint32))
        _check_calls(ctx.calls(capacity=CALL_CAP), vc[3], "the closing records")
    finally:
        ctx.close()


# ---- 5: m17hip_set_stream with a run in flight ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["torch_stream", "null_stream"])
@pytest.mark.parametrize("staged", [False, True], ids=["in_place", "staged"])
@pytest.mark.parametrize("kind", ["f32", "iq_i16", "iq_f32"])
def test_set_stream_then_the_next_run(f32_case, iq_cases, kind, staged, target):
    """m17hip_set_stream at once after run 0 was queued on the library's stream, then the next block and run 1 on the new stream: the float tail run 0
    carries and (IQ) the discriminator's carry must follow the run there.  `staged`: tuning key 16, the in-place producers write the staging slab on the
    copy stream (the payload stream); or not (the payload stream is the main stream and moves with it)."""
    import torch
    b = f32_case if kind == "f32" else iq_cases[kind[3:]]
    r = b.runs
    side = torch.cuda.Stream() if target == "torch_stream" else None
    ctx = m17hip.Context(CN, T0)
    try:
        up = ctx.upload if b.y is None else ctx.upload_iq
        if staged:
            ctx.tune(16, 1)
        up(b.x0)
        ctx.run()
        _in_flight(ctx)
        ctx.set_stream(side.cuda_stream if side is not None else 0)
        assert ctx.stream == (side.cuda_stream if side is not None else 0)
        up(b.x1["full"])
        ctx.run()
        _check_records(_frames_once(ctx), r.rec1["full"])
        _check_diag(ctx.diag(CN), r.diag1["full"], DIAG_STREAM)
        _check_words(ctx.download_f32(), _input_words(b, "full"), "the floats run 1 read")
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), r.rec0)
    finally:
        ctx.close()
        torch.cuda.synchronize()
