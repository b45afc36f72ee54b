"""GPU tests of host calls made while the TWO-STAGE TUNER is still in flight (ABI 610: m17hip_wide_config2).  tests/test_gpu_call_orders_wide.py rests on a
tuner that has left the device before the next host call (0.1 - 0.4 ms a staging at R = 2; the thing in flight there is a run on the main stream).  At
2.4 MSPS the two-stage tuner takes 22 - 25 times the demodulation step of as many samples: a live receiver's m17hip_upload_wide_async / _device_async return
with tune2_kernel, wide_carry_kernel and wide_hist_kernel queued on the copy stream and every later host call is made underneath them.  Here block 1 of every
case is staged and the call under test is made at once, with nothing synchronising in between; include/m17hip.h's promises for that situation are the cases:
m17hip_wide_channels never waits and a block already staged keeps its table, m17hip_wide_config / _config2 wait for the tuner's launches in flight,
m17hip_upload_wait blocks until the source has been left, blocks continue one another in call order across the two streams.

The regime is the parent modules': a fresh context per case (warmed and reset: see context()), a module fixture that makes the process's first staging
before any case, floats
(m17hip_download_f32) compared as uint32 words against the HOST form fed block by block (wide2_lib.Tuner2 through PFeeds2), records, m17_diag and counts byte
for byte against the float oracle on those floats (_frames_once, Expect).

Shape: 64 channels on two sources at 10 x 5 with the default taps (81 / 161); per source four FM transmissions from wide_lib.wideband, eight channels per
transmission 3 Hz apart (no two of the 64 share a frequency word); int16 sources, and uint8 ones where marked.  Block 1 has T1 outputs, the blocks behind it
384.  The context holds that set of 64 channels REP times over (channel c listens where channel c % 64 does): measured on the MI355X, the tuner of 64
channels takes 0.14 / 0.20 / 0.36 ms at 4800 / 9600 / 19200 outputs — the 50 ms on record are 64 sources x 64 channels EACH, 4096 channels — and from the
staging call to the return of the m17hip_demod_run behind it are 0.27 ms: with 64 channels no block of a size whose host form a CPU computes in seconds is
in flight when the next call is made.  The tuner's time goes with channels x outputs, the host form's with DISTINCT channels x outputs: the 64 distinct
channels are computed once on the CPU and every one of the context's channels is compared with its original, word for word and record for record.

The premise.  The copy stream has no accessor, so it cannot be asked.  A module fixture measures D on a throwaway context with m17hip_timing_enable: the
smallest of three single-launch readings of timing index 10 from three in-place device blocks of T1 outputs.  A case takes t_s = time.perf_counter() just
before the staging call, t_c just before the call under test and t_r when it returns: the tuner cannot end before t_s + D.  A call that must not wait has
t_r - t_s < 0.5 D; a call that must wait was made with t_c - t_s < 0.5 D and returned with t_r - t_s >= 0.5 D.  A case whose premise fails FAILS.  Timing is
off inside the cases.  T1 is the smallest of 4800, 9600 and 19200 outputs at which, with REP x 64 channels, D is at least eight times the longest t_r - t_s of the calls that do not
wait, measured once on the MI355X with the product build (NOTES.md has D and the intervals): the 0.5 D of the premise then keeps the parent's factor four.
"""
import copy
import time

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import test_gpu_call_orders_formats as par
import test_gpu_call_orders_wide as pw
import wide2_lib as w2
import wide_lib as wl
from test_gpu_call_orders_formats import CN, DIAG_STREAM, THREADS, Expect, _check_diag, _check_records, _check_words, _in_flight, _u32

pytestmark = pytest.mark.gpu

S, R1, R2 = 2, 10, 5
R = R1 * R2
T1 = 4800                    # outputs of block 1, whose tuner is in flight (chosen by the rule above)
TB = 384                     # outputs of the blocks behind it
TOTAL = 2 * T1 + TB          # outputs the sources hold: block 1, then T1 + 192 for the block that outgrows the raw buffer, or up to three of TB
REP = 64                     # times the 64 channels are held: 4096 channels, the shape the recorded 50.3 ms per 48 000 outputs belong to
ALL = CN * REP
T0F = par.T0 // 4            # samples of a float run 0 that keeps the main stream busy
OFFSETS = (-762500.0, -212500.0, 312500.0, 887500.0)   # Hz from the source's centre, inside the +-1.2 MHz a source covers
SRC, TX, PER_SOURCE, STEP_HZ, GROUPS = pw.SRC, pw.TX, pw.PER_SOURCE, pw.STEP_HZ, pw.GROUPS
FMTS, AMPLITUDE, SIGMA, SB, GAIN = pw.FMTS, pw.AMPLITUDE, pw.SIGMA, pw.SB, pw.GAIN
FCW = np.array([m17hip.wide_fcw(OFFSETS[TX[c]] + STEP_HZ * (c // (S * PER_SOURCE) + 8 * SRC[c]), R) for c in range(CN)], dtype=np.int64)
assert len(set(FCW.tolist())) == CN and T1 % 192 == 0 and TB % 192 == 0
TAPS1, TAPS2 = None, None    # (the default taps: from the library, on first use)
LISTED = par.FEED_AGAIN      # a third of the first 64 channels (their copies further up go on: a reset list of thousands is thousands of memsets)
# the configurations m17hip_wide_config2 / m17hip_wide_config replace 10 x 5 with
OTHER2 = (16, 1)             # default taps 129 / 33
OTHER1 = (16, 33)            # single stage: decimation, taps (a Hamming window of unit DC gain)


def taps():
    global TAPS1, TAPS2
    if TAPS1 is None:
        TAPS1, TAPS2 = m17hip.wide_default_taps2(R1, R2)
        assert (TAPS1.size, TAPS2.size) == (81, 161)
    return TAPS1, TAPS2


def table(k):
    """Table k = 1, 2, 3 beside the base table: another quarter of the channels on the other source, at the word of another transmission there, 50 Hz and
    more beside every word in use."""
    who = np.arange(k, CN, 4)
    src, fcw = SRC.copy(), FCW.copy()
    src[who] = 1 - src[who]
    fcw[who] = [m17hip.wide_fcw(OFFSETS[(TX[c] + 1 + k) % PER_SOURCE] + 50.0 + STEP_HZ * c, R) for c in who]
    assert len(set(fcw.tolist())) == CN
    return who, src, fcw


def rep(a):
    """Per-channel rows of the 64 distinct channels -> of all the context's channels."""
    a = np.asarray(a)
    return np.tile(a, (REP,) + (1,) * (a.ndim - 1))


def rep_rows(rows):
    """Expect.run's per-channel records of the 64 distinct channels -> one array for all channels, in channel order."""
    out = []
    for c in range(ALL):
        q = rows[c % CN].copy()
        q["channel"] = c
        out.append(q)
    return np.concatenate(out)


class PFeeds2(w2.Feeds2):
    """wide2_lib.Feeds2 with the channels of a block on a thread pool."""

    def block(self, a, b):
        def one(c):
            s = self.src[c]
            t = w2.Tuner2(*self.cfg, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            return t.block(self.data[s][a * self.R: b * self.R]), t.carry
        w2.lib()
        res = pw._pool(one, len(self.src))
        for c, (_, carry) in enumerate(res):
            self.carry[c] = carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][a * self.R: b * self.R])
        return np.stack([o for o, _ in res])


def feeds(x, src=SRC, fcw=FCW):
    return PFeeds2(x, *_cfg(), src, fcw, GAIN)


def _cfg():
    t1, t2 = taps()
    return t1, R1, t2, R2


def sources(fmt, seed=20261020):
    p = ol.gen_params(seed=seed, kind=-1, n_frames=max(TOTAL // 1920 - 3, 1), lead_in=48, total=TOTAL)
    bb = ol.generate_batch(p, S * PER_SOURCE, TOTAL, threads=THREADS)
    x = np.stack([wl.wideband(bb[PER_SOURCE * s: PER_SOURCE * (s + 1)], OFFSETS, R, amplitude=AMPLITUDE[fmt], sigma=SIGMA[fmt], seed=s + 1, fmt=fmt) for s in range(S)])
    x.setflags(write=False)
    return x


class Case:
    """The sources of one format in host, pinned and device memory; block 1's floats under the base table (y1) and under table 1 (y1_other), the feed's
    state behind block 1 (ref1: deep-copied by whoever continues it), and the float oracle's records for run 1 alone and behind a float run 0."""

    def __init__(self, fmt, x0f):
        import torch
        self.fmt, self.sb = fmt, SB[fmt]
        self.x = sources(fmt)
        ref = feeds(self.x)
        self.y1 = ref.block(0, T1)
        self.ref1 = ref
        _, src, fcw = table(1)
        self.y1_other = feeds(self.x, src, fcw).block(0, T1)
        assert np.isfinite(self.y1).all()
        for a in (self.y1, self.y1_other):
            a.setflags(write=False)
        self.pitch = TOTAL * R
        self.pin = torch.from_numpy(np.array(self.x)).pin_memory()
        self.dev = torch.from_numpy(np.array(self.x)).cuda()
        torch.cuda.synchronize()
        idle = Expect(np.ascontiguousarray(self.y1))
        self.idle = (None, rep_rows(idle.run(0, T1)), rep(idle.diags))
        busy = Expect(np.concatenate([x0f, self.y1], axis=1))
        self.busy = (rep_rows(busy.run(0, T0F)), rep_rows(busy.run(T0F, T0F + T1)), rep(busy.diags))
        assert self.idle[1].size > 0 and self.busy[0].size > ALL and self.busy[1].size > 0, "run 1 yields records"
        self.y1_all = rep(self.y1)
        self.y1_all.setflags(write=False)

    def at(self, where, a):
        """The pointer to output a's first sample in the pinned or the device copy."""
        base = self.pin.data_ptr() if where == "pinned" else self.dev.data_ptr()
        return base + a * R * self.sb

    def host(self, a, b):
        return np.ascontiguousarray(self.x[:, a * R: b * R])

    def behind_block_1(self, src=None, fcw=None):
        r = copy.deepcopy(self.ref1)
        if src is not None:
            r.src, r.fcw = list(src), list(fcw)
        return r


_SILENCE = {}


def context(fmt, maxT=T1):
    """A fresh context under the base table that has made its first in-place block, its first staging and two runs (of silence), and was then reset: the
    first staging of a context allocates its second slab pair, the second float slab and the copy stream and publishes the channel table — at 4096
    channels 0.3 to 1.4 GB of allocations, which took 0.1 ms as a rule and 29 ms once, inside the interval a case measures.  m17hip_demod_reset then
    starts the stream and the sources' feeds over: what a case sees is a fresh stream."""
    import torch
    if fmt not in _SILENCE:
        _SILENCE[fmt] = torch.zeros((S, TB * R, 2), dtype=torch.int16 if fmt == wl.IQ_I16 else torch.uint8, device="cuda")
        torch.cuda.synchronize()
    quiet = _SILENCE[fmt].data_ptr()
    ctx = m17hip.Context(ALL, maxT)
    try:
        ctx.wide_config2(S, R1, R2, fmt)
        ctx.wide_channels(rep(SRC), rep(FCW))
        ctx.upload_wide_device(quiet, ALL, TB, TB * R)
        ctx.run()
        ctx.upload_wide_device_async(quiet, ALL, TB, TB * R)
        ctx.run(channels=ALL, samples=TB)
        ctx.frames()
        ctx.upload_wait()
        ctx.reset()
    except Exception:
        ctx.close()
        raise
    return ctx


def _frames_once(ctx):
    """m17hip_frames_fetch ONCE with room for every record of every channel (the parent's, sized for this module's channels)."""
    import ctypes as C
    recs = np.zeros(ALL * par._rec_cap(T0F + T1), dtype=m17hip.FRAME_REC)
    got = C.c_uint64(0)
    ctx._chk(ctx.lib.m17hip_frames_fetch(ctx.h, m17hip._ptr(recs), C.c_uint64(recs.size), C.byref(got)))
    return recs[: got.value]


def _words(got, exp64, what):
    _check_words(got, rep(exp64), what)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def first_staging_of_the_process():
    """The parent modules' throwaway staging, and one two-stage block in place, one retune and one staged block: the copy stream, the pinned staging of a
    channel table and both of its device copies have been allocated once in this process before any case is timed."""
    import torch
    x = np.zeros((ALL, 2 * TB), dtype=np.int16)
    pin = torch.from_numpy(x.copy()).pin_memory()
    ctx = m17hip.Context(ALL, 2 * TB)
    try:
        ctx.upload(x)
        ctx.run()
        ctx.upload_async(pin.data_ptr(), ALL, 2 * TB)
        ctx.run(channels=ALL, samples=2 * TB)
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()
    w = np.zeros((S, TB * R, 2), dtype=np.int16)
    wpin = torch.from_numpy(w.copy()).pin_memory()
    ctx = context(wl.IQ_I16, TB)
    try:
        ctx.upload_wide(w)   # (the host forms' raw buffer and a pinned block as well)
        ctx.run()
        ctx.wide_channels(rep(SRC[::-1].copy()), rep(FCW))
        ctx.upload_wide_async(wpin.data_ptr(), ALL, TB, TB * R)
        ctx.run(channels=ALL, samples=TB)
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def run0_floats():
    """A float run 0 of 24 000 samples (the head of the parent's float stream) for every channel: the 64 rows on the host, all rows on the device."""
    import torch
    x = np.ascontiguousarray(fl.off_grid(par.baseband(), seed=607)[:, :T0F])
    x.setflags(write=False)
    dev = torch.from_numpy(np.array(x)).cuda().repeat(REP, 1).contiguous()
    torch.cuda.synchronize()
    return x, dev


@pytest.fixture(scope="module")
def cases(run0_floats):
    return {name: Case(f, run0_floats[0]) for name, f in FMTS.items()}


@pytest.fixture(scope="module")
def tuner_s(cases, first_staging_of_the_process):
    """D per format, in seconds: the smallest of three single-launch readings of timing index 10 on a throwaway context."""
    out = {}
    for name, b in cases.items():
        ctx = context(b.fmt)
        try:
            ctx.timing(True)
            reads = []
            for _ in range(3):
                ctx.timing_reset()
                ctx.upload_wide_device(b.at("device", 0), ALL, T1, b.pitch, GAIN)
                ms, launches = ctx.timing_get("tune2")
                assert launches == 1 and ms > 0
                reads.append(ms)
            ctx.timing(False)
        finally:
            ctx.close()
        out[name] = 1e-3 * min(reads)
        print(f"[wide2] D ({name}, {T1} outputs): {min(reads):.3f} ms (readings {', '.join(f'{r:.3f}' for r in reads)})")
    return out


# ---- the steps of a case -------------------------------------------------------------------------------------------------------------------------
NOT_A_PASS = "this case cannot show an ordering error (not a pass)"


def _stage_1(ctx, b, form):
    """Block 1, staged: its tuner runs on the copy stream.  Returns t_s."""
    t_s = time.perf_counter()
    if form == "pinned":
        ctx.upload_wide_async(b.at("pinned", 0), ALL, T1, b.pitch, GAIN)
    else:
        ctx.upload_wide_device_async(b.at("device", 0), ALL, T1, b.pitch, GAIN)
    return t_s


def _made_under_the_tuner(t_s, D, what, t_c=None):
    """The premise of a call made at t_c (default: now): block 1's tuner, which cannot end before t_s + D, had more than half of its time left."""
    t_c = time.perf_counter() if t_c is None else t_c
    print(f"[wide2] {what}: made {1e3 * (t_c - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_c - t_s < 0.5 * D, f"{what} was made {1e3 * (t_c - t_s):.3f} ms after the staging call began, the tuner takes {1e3 * D:.3f} ms: it may have finished on " \
                                f"the device before the call under test was made: {NOT_A_PASS}"
    return t_c


def _returned_under_the_tuner(t_s, D, what):
    """A call that must not wait has returned: t_r - t_s < 0.5 D (which says as well that it was made under the tuner)."""
    t_r = time.perf_counter()
    print(f"[wide2] {what}: returned {1e3 * (t_r - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_r - t_s < 0.5 * D, f"{what} returned {1e3 * (t_r - t_s):.3f} ms after the staging call began, the tuner takes {1e3 * D:.3f} ms: either it waited, or the " \
                                f"tuner may have finished on the device before the call under test was made: {NOT_A_PASS}"


def _waited(t_s, t_c, D, what, t_r=None):
    """A call that must wait for the tuner's launches in flight has returned (at t_r; default: now): it was made under the tuner and came back no earlier
    than half of D."""
    t_r = time.perf_counter() if t_r is None else t_r
    print(f"[wide2] {what}: made {1e3 * (t_c - t_s):.3f} ms, returned {1e3 * (t_r - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_c - t_s < 0.5 * D, f"{what} was made {1e3 * (t_c - t_s):.3f} ms after the staging call began, the tuner takes {1e3 * D:.3f} ms: {NOT_A_PASS}"
    assert t_r - t_s >= 0.5 * D, f"{what} returned {1e3 * (t_r - t_s):.3f} ms after the staging call began: it did not wait for a tuner that takes {1e3 * D:.3f} ms"


def _run_1_is(ctx, b, expect):
    """Run 1's records and m17_diag byte for byte (the float oracle on the host form's floats), then — with run 0 in front — run 0's."""
    rec0, rec1, diag = expect
    assert ctx.frames_count() == rec1.size
    _check_records(_frames_once(ctx), rec1)
    _check_diag(ctx.diag(ALL), diag, DIAG_STREAM)
    if rec0 is not None:
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), rec0)
        ctx.frames_select(0)


# ---- 1: m17hip_demod_run at once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,form,main", [("i16", "pinned", "idle"), ("i16", "pinned", "run_0"), ("i16", "device", "idle"), ("i16", "device", "run_0"),
                                           ("u8", "device", "idle"), ("u8", "device", "run_0")])
def test_run_at_once_behind_the_staging(cases, tuner_s, run0_floats, fmt, form, main):
    """m17hip_demod_run returns under the tuner; what it queued waited for the staging: run 1's records and diagnostics are the float oracle's on block 1's
    floats — the only check there is that the run waited — and the floats, fetched afterwards, the host form's.  (What a staged run waits for is
    ev_in_ready, which begin_staged records on the copy stream behind the tuner, not ev_copy: moving ev_copy in front of the tuner does not show here.)
    With the main stream idle, and with a float run 0 of 24 000 samples in flight on it (asserted)."""
    b, D = cases[fmt], tuner_s[fmt]
    busy = main == "run_0"
    ctx = context(b.fmt, T0F if busy else T1)
    try:
        if busy:
            ctx.upload_device(run0_floats[1].data_ptr(), ALL, T0F, dtype=np.float32)
            ctx.run()
            _in_flight(ctx)
        t_s = _stage_1(ctx, b, form)
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, D, f"m17hip_demod_run ({form}, {main})")
        _run_1_is(ctx, b, b.busy if busy else b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "the floats run 1 read")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 2: run, then block 2 in place on the main stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("form", ["host", "device"])
def test_run_then_block_2_in_place_at_once(cases, tuner_s, form, fmt):
    """Block 1 staged (from pinned memory in front of a host block, from device memory in front of a device block), its run, and block 2 tuned in place on
    the MAIN stream at once: its words continue block 1 — the sources' histories, the count and the channels' carries crossed from the copy stream through
    ev_iq alone.  (An in-place block is written into the slab run 1 reads, behind it: block 1's floats are gone by then and run 1's records stand for them.)"""
    b, D = cases[fmt], tuner_s[fmt]
    e2 = b.behind_block_1().block(T1, T1 + TB)
    fresh = feeds(b.x[:, T1 * R:]).block(0, 4)
    assert (_u32(fresh[:, 0]) != _u32(e2[:, 0])).all() and (_u32(fresh[:, 1:]) != _u32(e2[:, 1:4])).any(), "block 2's first floats are the ones carry and history decide"
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "pinned" if form == "host" else "device")
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, D, f"m17hip_demod_run in front of an in-place block ({form})")
        if form == "host":
            ctx.upload_wide(b.host(T1, T1 + TB), gain=GAIN)
        else:
            ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, in place behind a staged block")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


def test_block_2_in_place_at_once_before_block_1s_run(cases, tuner_s):
    """Block 2 tuned in place on the main stream at once behind the staging, BEFORE block 1's run: nothing but ev_iq stands between the two tuners (with
    the run in between, the main stream is behind the staging through the run, and upload_wide's own wait for ev_iq is redundant: the case above passes
    without it).  Blocks continue one another in call order: block 2's words continue block 1; run 1 then reads the staged block 1, untouched."""
    b, D = cases["i16"], tuner_s["i16"]
    e2 = b.behind_block_1().block(T1, T1 + TB)
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, D, "m17hip_upload_wide_device in front of the staged block's run")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, in place behind a staged block that has not run")
        ctx.run(channels=ALL, samples=T1)
        ctx.T = T1
        _check_words(ctx.download_f32(), b.y1_all, "block 1, run behind block 2's upload")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: m17hip_wide_channels at once ---------------------------------------------------------------------------------------------------------------
def test_retune_at_once_behind_the_staging(cases, tuner_s):
    """m17hip_wide_channels "never waits for anything in flight": it returns under the tuner.  "A block already staged keeps the table it was tuned with":
    block 1 has the base table's words, which differ from table 1's on every moved channel; block 2, in place, has table 1's."""
    b, D = cases["i16"], tuner_s["i16"]
    who, src, fcw = table(1)
    assert (_u32(b.y1[who]) != _u32(b.y1_other[who])).any(axis=1).all()
    e2 = b.behind_block_1(src, fcw).block(T1, T1 + TB)
    assert (_u32(e2[who]) != _u32(b.behind_block_1().block(T1, T1 + TB)[who])).any(axis=1).all()
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_channels(rep(src), rep(fcw))
        _returned_under_the_tuner(t_s, D, "m17hip_wide_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the retune")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, in place behind the retune")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_retunes_back_to_back_each_table_copy_rewritten_under_tuners(cases, tuner_s):
    """Two retunes back to back behind the staging, the run, a staged block 2 (it publishes table 2 into the device copy block 1's tuner does NOT read), a
    third retune, the run, a staged block 3 (table 3 goes into the copy block 1 read): each device copy is rewritten while tuners that read it were queued.
    Block 1 has the base table's words, block 2 table 2's, block 3 table 3's."""
    b, D = cases["i16"], tuner_s["i16"]
    tables = [table(k) for k in (1, 2, 3)]
    ref = b.behind_block_1(*tables[1][1:])
    e2 = ref.block(T1, T1 + TB)
    ref.src, ref.fcw = list(tables[2][1]), list(tables[2][2])
    e3 = ref.block(T1 + TB, T1 + 2 * TB)
    assert (_u32(e2[tables[1][0]]) != _u32(b.behind_block_1(*tables[0][1:]).block(T1, T1 + TB)[tables[1][0]])).any(axis=1).all(), "table 2, not table 1"
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_channels(rep(tables[0][1]), rep(tables[0][2]))
        ctx.wide_channels(rep(tables[1][1]), rep(tables[1][2]))
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, D, "two retunes back to back and m17hip_demod_run")
        ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)   # (queued behind block 1's tuner: stream order)
        ctx.wide_channels(rep(tables[2][1]), rep(tables[2][2]))
        ctx.T = T1                                                                  # (the latest run's input, not the block staged since)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before every retune")
        ctx.T = TB
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), e2, "block 2, staged under table 2")
        ctx.upload_wide_async(b.at("pinned", T1 + TB), ALL, TB, b.pitch, GAIN)
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), e3, "block 3, staged under table 3")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4: resets at once -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", ["in_place", "staged"])
def test_channel_reset_at_once_behind_the_staging(cases, tuner_s, second):
    """m17hip_demod_reset_channels for a third of the channels at once behind the staging: the carries are zeroed behind block 1's tuner, on its stream.
    Block 1 is untouched; block 2 — in place on the main stream, or staged — has +0 as the listed channels' first output and continues every other channel
    (the copies of the listed channels further up in the context among them)."""
    b, D = cases["i16"], tuner_s["i16"]
    ref = b.behind_block_1()
    for c in LISTED:
        ref.carry[c] = np.zeros(2, dtype=np.float32)
    e2 = ref.block(T1, T1 + TB)
    plain = b.behind_block_1().block(T1, T1 + TB)
    rest = np.delete(np.arange(CN), LISTED)
    assert (e2[LISTED, 0] == 0).all() and (plain[LISTED, 0] != 0).all() and np.array_equal(_u32(e2[rest]), _u32(plain[rest]))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.reset_channels(LISTED)
        _returned_under_the_tuner(t_s, D, "m17hip_demod_reset_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the reset")
        if second == "in_place":
            ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        else:
            ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)
            ctx.run(channels=ALL, samples=TB)
        every = rep(plain)   # (the listed channels are among the first 64: their copies further up go on)
        every[:CN] = e2
        _check_words(ctx.download_f32(), every, f"block 2 ({second}) behind the reset")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_reset_at_once_behind_the_run(cases, tuner_s):
    """m17hip_demod_reset at once behind block 1's run: block 2 starts from zero histories, a zero count and zero carries — a fresh host form."""
    b, D = cases["i16"], tuner_s["i16"]
    e2 = feeds(b.x[:, T1 * R:]).block(0, TB)
    assert not np.array_equal(_u32(e2), _u32(b.behind_block_1().block(T1, T1 + TB)))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.run(channels=ALL, samples=T1)
        _made_under_the_tuner(t_s, D, "m17hip_demod_reset")
        ctx.reset()
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2 behind m17hip_demod_reset")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: another configuration at once ----------------------------------------------------------------------------------------------------------------
def _reconfigure(ctx, b, to):
    """The call under test, and block 2's expectation: a fresh feed of the new configuration over the samples behind block 1, the carries kept."""
    carries = [c.copy() for c in b.ref1.carry]
    rest = b.x[:, T1 * R:]
    if to == "config2":
        t1, t2 = m17hip.wide_default_taps2(*OTHER2)
        assert (t1.size, t2.size) == (129, 33)
        new = PFeeds2(rest, t1, OTHER2[0], t2, OTHER2[1], SRC, FCW, GAIN)
        call = lambda: ctx.wide_config2(S, OTHER2[0], OTHER2[1], b.fmt)
        rate = OTHER2[0] * OTHER2[1]
    else:
        h = wl.hamming_taps(OTHER1[1])
        new = pw.PFeeds(rest, h, SRC, FCW, OTHER1[0], GAIN)
        call = lambda: ctx.wide_config(S, OTHER1[0], b.fmt, h)
        rate = OTHER1[0]
    plain = copy.deepcopy(new).block(0, 4)
    new.carry = carries
    e2 = new.block(0, TB)
    assert (_u32(plain[:, 0]) != _u32(e2[:, 0])).all() and np.array_equal(_u32(plain[:, 1:]), _u32(e2[:, 1:4])), "the carries are kept, the sources start over"
    assert TB * rate <= (TOTAL - T1) * R
    return call, e2


@pytest.mark.parametrize("where", ["before_its_run", "behind_its_run"])
@pytest.mark.parametrize("to", ["config2", "config"])
def test_reconfiguration_at_once_waits_for_the_tuner(cases, tuner_s, to, where):
    """m17hip_wide_config2 (to 16 x 1, 129 / 33 taps) and m17hip_wide_config (to a single stage) "wait for the tuner's launches in flight": made at once
    behind the staging BEFORE its run, and at once behind its run, the call returns no earlier than the tuner can (its buffers go).  Run 1's floats and
    records are the old configuration's; block 2 is a fresh feed of the new one with the carries block 1 left."""
    b, D = cases["i16"], tuner_s["i16"]
    ctx = context(b.fmt)
    try:
        call, e2 = _reconfigure(ctx, b, to)
        t_s = _stage_1(ctx, b, "device")
        if where == "behind_its_run":
            ctx.run(channels=ALL, samples=T1)
        t_c = time.perf_counter()
        call()
        _waited(t_s, t_c, D, f"m17hip_wide_{to} {where}")
        if where == "before_its_run":
            ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, tuned with the configuration before")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, a fresh feed of the new configuration")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 6: the raw buffer grows -------------------------------------------------------------------------------------------------------------------------
def test_raw_buffer_grows_behind_a_pinned_block_in_flight(cases, tuner_s):
    """Block 1 from pinned memory goes through the context's raw buffer (sized for T1 outputs) and its tuner reads it; its run, then an in-place HOST block
    of T1 + 192 outputs at once: the buffer is reallocated.  Block 2's words are exact, and block 1's stand behind run 1's records and diagnostics (the
    in-place block has overwritten its floats)."""
    b, D = cases["i16"], tuner_s["i16"]
    n2 = T1 + 192
    e2 = b.behind_block_1().block(T1, T1 + n2)
    ctx = context(b.fmt, n2)
    try:
        t_s = _stage_1(ctx, b, "pinned")
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, D, "m17hip_demod_run in front of the block that outgrows the raw buffer")
        ctx.upload_wide(b.host(T1, T1 + n2), gain=GAIN)
        _words(ctx.download_f32(), e2, "block 2, longer than the raw buffer was")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 7: m17hip_upload_wait at once -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pinned", "device"])
def test_upload_wait_at_once_then_the_source_overwritten(cases, tuner_s, form):
    """m17hip_upload_wait blocks until the source buffer has been left: it returns no earlier than the tuner can.  The source (a copy of this case's own) is
    then overwritten — a numpy fill of the pinned block, fill_ on a torch stream and a synchronise for the device block — and run 1's floats and records
    are still block 1's."""
    import torch
    b, D = cases["i16"], tuner_s["i16"]
    mine = b.pin.clone().pin_memory() if form == "pinned" else b.dev.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = context(b.fmt)
    try:
        t_s = time.perf_counter()
        if form == "pinned":
            ctx.upload_wide_async(mine.data_ptr(), ALL, T1, b.pitch, GAIN)
        else:
            ctx.upload_wide_device_async(mine.data_ptr(), ALL, T1, b.pitch, GAIN)
        t_c = time.perf_counter()
        ctx.upload_wait()
        t_r = time.perf_counter()
        if form == "pinned":
            mine.numpy().fill(77)
        else:
            with torch.cuda.stream(side):
                mine.fill_(77)
            side.synchronize()
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, its source overwritten behind m17hip_upload_wait")
        _run_1_is(ctx, b, b.idle)
        _waited(t_s, t_c, D, f"m17hip_upload_wait ({form})", t_r)   # (the comparisons first: a source overwritten under the tuner would show in the words)
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---- 8: m17hip_set_stream at once --------------------------------------------------------------------------------------------------------------------
def test_set_stream_at_once_then_the_run_on_the_new_stream(cases, tuner_s):
    """m17hip_set_stream to a torch stream at once behind the staging, then run 1 on that stream: it still waits for the staging."""
    import torch
    b, D = cases["i16"], tuner_s["i16"]
    side = torch.cuda.Stream()
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, D, "m17hip_set_stream")
        ctx.set_stream(side.cuda_stream)
        assert ctx.stream == side.cuda_stream
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "the floats run 1 read on the new stream")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), b.behind_block_1().block(T1, T1 + TB), "block 2, in place on the new stream")
        ctx.upload_wait()
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---- 9: a narrowband block at once behind the run ----------------------------------------------------------------------------------------------------
def test_narrowband_block_at_once_behind_the_run(cases, tuner_s):
    """m17hip_upload_iq_device, in place on the main stream, at once behind block 1's run: the discriminator takes each channel's first output against the
    tuner's last z, which wide_carry_kernel leaves on the copy stream."""
    b, D = cases["i16"], tuner_s["i16"]
    rng = np.random.default_rng(6130)
    z = rng.integers(-20000, 20001, size=(CN, TB, 2)).astype(np.int16)
    zdev = pw_dev(rep(z))
    e = np.stack([iq.discriminate(z[c], 1.0, b.ref1.carry[c])[0] for c in range(CN)])
    zero = np.stack([iq.discriminate(z[c, :4], 1.0, None)[0] for c in range(CN)])
    assert (_u32(zero[:, 0]) != _u32(e[:, 0])).all() and np.array_equal(_u32(zero[:, 1:]), _u32(e[:, 1:4]))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.run(channels=ALL, samples=T1)
        _made_under_the_tuner(t_s, D, "m17hip_upload_iq_device")
        ctx.upload_iq_device(zdev.data_ptr(), ALL, TB, pitch=TB, iq_format=iq.IQ_I16)
        _words(ctx.download_f32(), e, "a narrowband block behind a two-stage block in flight")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


def pw_dev(a):
    """The array on the device, complete when this returns."""
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


# ---- 10: close() at once -----------------------------------------------------------------------------------------------------------------------------
def test_close_at_once_then_a_fresh_context_on_the_parked_streams(cases, tuner_s):
    """m17hip_ctx_destroy at once behind the staging; the next fresh context takes the stream set the closed one parked and tunes one small block to the
    host form's words."""
    b, D = cases["i16"], tuner_s["i16"]
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, D, "m17hip_ctx_destroy")
    finally:
        ctx.close()
    ctx = context(b.fmt)
    try:
        ctx.upload_wide_device_async(b.at("device", 0), ALL, TB, b.pitch, GAIN)
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), b.y1[:, :TB], "a small block on a fresh context")
        ctx.upload_wait()
    finally:
        ctx.close()
