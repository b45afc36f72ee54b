"""GPU tests of host calls made while the RESAMPLING TUNER is still in flight (ABI 615: m17hip_wide_resample, resample_kernel).  The regime is
tests/test_gpu_call_orders_wide2.py's, whose helpers, fixtures and parents' are imported as they stand: block 1 of every case is staged and the call under
test is made at once, with nothing synchronising in between; a fresh context per case (warmed and reset: context()); that module's first staging of the
process before any case; floats (m17hip_download_f32) compared as uint32 words against the HOST form fed the same blocks (resample_lib.Feeds, the channels
of a block on a thread pool); records, m17_diag and counts byte for byte against the float oracle on those floats.  Most of the ordering code under these
calls is shared with the other tuners (launch_tune, wide_after_block, upload_frame); the resampler's own is m17hip_wide_resample through wide_setup with up
and down, which must wait for launches in flight, a raw buffer sized by rows of T / up * down * decim1 samples, and a history of
(ceil(ntaps2 / up) - 1) decim1 + ntaps1 - 1 samples a source.

Shape: 2 int16 sources at 2.048 MSPS (16 x 3 / 8) with the default taps (129 / 257); per source four FM transmissions at the parent's offsets (inside
+-1.0 MHz of the +-1.024 MHz a source covers), made as tests/test_resample_input.py's source_2048k makes its source — at 128 x 48 kSPS, every third sample
kept, that module's noise added at the thinned rate; the clipped share is asserted under its cap —; 64 distinct channels, eight per transmission 3 Hz apart,
held REP = 64 times over (4096 channels: channel c listens where channel c % 64 does) as in the parent, every one compared with its original.  Block 1 has
T1 outputs, the blocks behind it 384.

The premise is the parent's: D is the smallest of three single-launch readings of the timer "resample" on a throwaway context at T1 outputs; t_s just before
the staging call, t_c just before the call under test, t_r when it returns.  A call that must not wait has t_r - t_s < 0.5 D; one that must wait was made
with t_c - t_s < 0.5 D and returned with t_r - t_s >= 0.5 D.  A case whose premise fails FAILS.  Timing is off inside the cases.  T1 is the smallest of
4800, 9600 and 19200 outputs at which D is at least eight times the longest t_r - t_s of the calls that do not wait, measured on the MI355X with the product
build (NOTES.md has D and the intervals per family).  Where a two-stage block is the one in flight
(test_wide_resample_at_once_under_a_two_stage_block_in_flight), D is the timer "tune2"'s.
"""
import copy
import ctypes as C
import time

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import resample_lib as rl
import test_gpu_call_orders_formats as par
import test_gpu_call_orders_wide as pw
import test_gpu_call_orders_wide2 as p2
import test_resample_input as cpu
import wide_lib as wl
from test_gpu_call_orders_formats import CN, DIAG_STREAM, THREADS, Expect, _check_diag, _check_records, _check_words, _in_flight, _u32
from test_gpu_call_orders_wide2 import (ALL, GAIN, LISTED, OFFSETS, PER_SOURCE, REP, SRC, STEP_HZ, T0F, TB, TX, _made_under_the_tuner,   # noqa: F401
                                        _returned_under_the_tuner, _waited, first_staging_of_the_process, rep, rep_rows, run0_floats)

pytestmark = pytest.mark.gpu

S, R1, U, D = 2, 16, 3, 8
GROUP = R1 * D               # samples of a source under U outputs
RATIO = GROUP / U            # samples per output: 2.048 MSPS
T1 = 4800                    # outputs of block 1, whose tuner is in flight (chosen by the rule above)
TOTAL = 2 * T1 + TB          # outputs the sources hold: block 1, then T1 + 192 for the block that outgrows the raw buffer, or blocks of TB
FMT, SB = wl.IQ_I16, 4
FCW = np.array([m17hip.wide_fcw(OFFSETS[TX[c]] + STEP_HZ * (c // (S * PER_SOURCE) + 8 * SRC[c]), RATIO) for c in range(CN)], dtype=np.int64)
assert len(set(FCW.tolist())) == CN and T1 % 192 == 0 and TB % 192 == 0 and TOTAL % U == 0 and max(abs(f) for f in OFFSETS) < 1.0e6
TAPS = {}                    # (the default taps of a shape: from the library, on first use)
OTHER_R = (5, 12, 125)       # the ratio m17hip_wide_resample replaces 16 x 3 / 8 with: 2.5 MSPS, default taps 41 / 4001, a tile of 47 groups
OTHER2 = p2.OTHER2           # ... and m17hip_wide_config2: 16 x 1, default taps 129 / 33
UNDER2 = (16, 2)             # the two-stage shape that is in flight where m17hip_wide_resample is the call under it: default taps 129 / 65


def taps(shape=(R1, U, D)):
    if shape not in TAPS:
        TAPS[shape] = m17hip.wide_resample_default_taps(*shape)
    return TAPS[shape]


def rows(n, shape=(R1, U, D)):
    """Samples of a source under n outputs."""
    return rl.row_len(n, *shape)


def table(k):
    """The parent's table k beside the base table, in this shape's frequency words."""
    who = np.arange(k, CN, 4)
    src, fcw = SRC.copy(), FCW.copy()
    src[who] = 1 - src[who]
    fcw[who] = [m17hip.wide_fcw(OFFSETS[(TX[c] + 1 + k) % PER_SOURCE] + 50.0 + STEP_HZ * c, RATIO) for c in who]
    assert len(set(fcw.tolist())) == CN
    return who, src, fcw


class PFeeds(rl.Feeds):
    """resample_lib.Feeds with the channels of a block on the parent's thread pool."""

    def block(self, a, b):
        lo, hi = rl.row_len(a, self.R1, self.U, self.D), rl.row_len(b, self.R1, self.U, self.D)

        def one(c):
            s = self.src[c]
            t = rl.Resampler(*self.cfg, int(self.fcw[c]), self.gain, count=self.per_source[s].count)
            t.hist[:] = self.per_source[s].hist
            t.carry[:] = self.carry[c]
            return t.block(self.data[s][lo:hi]), t.carry
        rl.lib()
        res = pw._pool(one, len(self.src))
        for c, (_, carry) in enumerate(res):
            self.carry[c] = carry
        for s in range(len(self.data)):
            self.per_source[s].block(self.data[s][lo:hi])
        return np.stack([o for o, _ in res])


def feeds(x, src=SRC, fcw=FCW, shape=(R1, U, D)):
    t1, t2 = taps(shape)
    return PFeeds(x, t1, shape[0], shape[1], shape[2], t2, src, fcw, GAIN)


def sources(seed=20261020):
    """x[S] int16 rows of TOTAL outputs: four transmissions each, at 128 x 48 kSPS and every third sample kept (a constant-envelope signal may be thinned),
    test_resample_input's noise added at the thinned rate, rounded."""
    p = ol.gen_params(seed=seed, kind=-1, n_frames=max(TOTAL // 1920 - 3, 1), lead_in=48, total=TOTAL)
    bb = ol.generate_batch(p, S * PER_SOURCE, TOTAL, threads=THREADS)
    out = []
    for s in range(S):
        z = wl.wideband(bb[PER_SOURCE * s: PER_SOURCE * (s + 1)], OFFSETS, GROUP, fmt=wl.IQ_F32, sigma=0.0)[::U].astype(np.complex128)
        assert z.size == rows(TOTAL)
        rng = np.random.default_rng(s + 1)
        z = z + cpu.SIGMA * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size))
        out.append(np.clip(np.rint(np.stack([z.real, z.imag], axis=-1)), -32768, 32767).astype(np.int16))
    x = np.stack(out)
    clipped = float(((x == -32768) | (x == 32767)).any(axis=-1).mean())
    assert clipped <= cpu.CLIPPED_CAP, clipped
    x.setflags(write=False)
    return x


class Case:
    """The sources in host, pinned and device memory; block 1's floats under the base table (y1) and under table 1 (y1_other), the feed's state behind
    block 1 (ref1: deep-copied by whoever continues it), and the float oracle's records for run 1 alone and behind a float run 0."""

    def __init__(self, x0f):
        import torch
        assert rl.tile(129, R1, 257, U, D) == cpu.TILES[(R1, U, D, 129, 257)] and rl.tile(41, 5, 4001, 12, 125) == cpu.TILES[(5, 12, 125, 41, 4001)]
        self.x = sources()
        ref = feeds(self.x)
        self.y1 = ref.block(0, T1)
        self.ref1 = ref
        _, src, fcw = table(1)
        self.y1_other = feeds(self.x, src, fcw).block(0, T1)
        assert np.isfinite(self.y1).all()
        for a in (self.y1, self.y1_other):
            a.setflags(write=False)
        self.pitch = rows(TOTAL)
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
        """The pointer to the first sample under output a (a multiple of `up`) in the pinned or the device copy."""
        base = self.pin.data_ptr() if where == "pinned" else self.dev.data_ptr()
        return base + rows(a) * SB

    def host(self, a, b):
        return np.ascontiguousarray(self.x[:, rows(a): rows(b)])

    def behind_block_1(self, src=None, fcw=None):
        r = copy.deepcopy(self.ref1)
        if src is not None:
            r.src, r.fcw = list(src), list(fcw)
        return r


_SILENCE = []


def context(maxT=T1, two_stage=None):
    """The parent's context() under the resampler (or, with `two_stage` = (decim1, decim2), under the two-stage tuner): a fresh context under the base table
    that has made its first in-place block, its first staging and two runs of silence, and was then reset — no allocation of the first staging lies
    inside the interval a case measures, and what a case sees is a fresh stream."""
    import torch
    if not _SILENCE:
        _SILENCE.append(torch.zeros((S, rows(TB), 2), dtype=torch.int16, device="cuda"))
        torch.cuda.synchronize()
    quiet, pitch = _SILENCE[0].data_ptr(), rows(TB)
    ctx = m17hip.Context(ALL, maxT)
    try:
        if two_stage is None:
            ctx.wide_resample(S, R1, U, D, FMT)
        else:
            assert TB * two_stage[0] * two_stage[1] <= pitch
            ctx.wide_config2(S, two_stage[0], two_stage[1], FMT)
        ctx.wide_channels(rep(SRC), rep(FCW))
        ctx.upload_wide_device(quiet, ALL, TB, pitch)
        ctx.run()
        ctx.upload_wide_device_async(quiet, ALL, TB, pitch)
        ctx.run(channels=ALL, samples=TB)
        ctx.frames()
        ctx.upload_wait()
        ctx.reset()
    except Exception:
        ctx.close()
        raise
    return ctx


def _frames_once(ctx):
    """m17hip_frames_fetch ONCE with room for every record of every channel (the parent's, sized for this module's block 1)."""
    recs = np.zeros(ALL * par._rec_cap(T0F + T1), dtype=m17hip.FRAME_REC)
    got = C.c_uint64(0)
    ctx._chk(ctx.lib.m17hip_frames_fetch(ctx.h, m17hip._ptr(recs), C.c_uint64(recs.size), C.byref(got)))
    return recs[: got.value]


def _words(got, exp64, what):
    _check_words(got, rep(exp64), what)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(run0_floats):
    return Case(run0_floats[0])


def _measure(ctx, timer, upload):
    ctx.timing(True)
    reads = []
    for _ in range(3):
        ctx.timing_reset()
        upload()
        ms, launches = ctx.timing_get(timer)
        assert launches == 1 and ms > 0
        reads.append(ms)
    ctx.timing(False)
    return reads


@pytest.fixture(scope="module")
def tuner_s(case, first_staging_of_the_process):
    """D in seconds: the smallest of three single-launch readings of the timer "resample" on a throwaway context."""
    ctx = context()
    try:
        reads = _measure(ctx, "resample", lambda: ctx.upload_wide_device(case.at("device", 0), ALL, T1, case.pitch, GAIN))
    finally:
        ctx.close()
    print(f"[resample] D ({T1} outputs): {min(reads):.3f} ms (readings {', '.join(f'{r:.3f}' for r in reads)})")
    return 1e-3 * min(reads)


@pytest.fixture(scope="module")
def tuner2_s(case, first_staging_of_the_process):
    """D of the two-stage block at UNDER2, likewise from the timer "tune2"."""
    ctx = context(two_stage=UNDER2)
    try:
        reads = _measure(ctx, "tune2", lambda: ctx.upload_wide_device(case.at("device", 0), ALL, T1, case.pitch, GAIN))
    finally:
        ctx.close()
    print(f"[resample] D of tune2_kernel at {UNDER2[0]} x {UNDER2[1]} ({T1} outputs): {min(reads):.3f} ms (readings {', '.join(f'{r:.3f}' for r in reads)})")
    return 1e-3 * min(reads)


# ---- the steps of a case -------------------------------------------------------------------------------------------------------------------------
def _stage_1(ctx, b, form):
    """Block 1, staged: its tuner runs on the copy stream.  Returns t_s."""
    t_s = time.perf_counter()
    if form == "pinned":
        ctx.upload_wide_async(b.at("pinned", 0), ALL, T1, b.pitch, GAIN)
    else:
        ctx.upload_wide_device_async(b.at("device", 0), ALL, T1, b.pitch, GAIN)
    return t_s


def _run_1_is(ctx, expect):
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
@pytest.mark.parametrize("form,main", [("pinned", "idle"), ("pinned", "run_0"), ("device", "idle"), ("device", "run_0")])
def test_run_at_once_behind_the_staging(case, tuner_s, run0_floats, form, main):
    """m17hip_demod_run returns under the tuner; what it queued waited for the staging: run 1's records and diagnostics are the float oracle's on block 1's
    floats, and the floats, fetched afterwards, the host form's.  With the main stream idle, and with a float run 0 of 24 000 samples in flight on it
    (asserted)."""
    b, Dt = case, tuner_s
    busy = main == "run_0"
    ctx = context(T0F if busy else T1)
    try:
        if busy:
            ctx.upload_device(run0_floats[1].data_ptr(), ALL, T0F, dtype=np.float32)
            ctx.run()
            _in_flight(ctx)
        t_s = _stage_1(ctx, b, form)
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, Dt, f"m17hip_demod_run ({form}, {main})")
        _run_1_is(ctx, b.busy if busy else b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "the floats run 1 read")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 2: block 2 in place at once, before block 1's run ---------------------------------------------------------------------------------------------
def test_block_2_in_place_at_once_before_block_1s_run(case, tuner_s):
    """Block 2 tuned in place on the main stream at once behind the staging, BEFORE block 1's run: nothing but ev_iq stands between the two tuners (the
    case that caught the missing iq_order wait in the parent).  Block 2's words continue block 1 — the sources' histories of 1488 samples, the count and the
    channels' carries crossed from the copy stream —; run 1 then reads the staged block 1, untouched."""
    b, Dt = case, tuner_s
    e2 = b.behind_block_1().block(T1, T1 + TB)
    fresh = feeds(b.x[:, rows(T1):]).block(0, U * 4)
    assert (_u32(fresh[:, 0]) != _u32(e2[:, 0])).all() and (_u32(fresh[:, 1:]) != _u32(e2[:, 1:U * 4])).any(), "block 2's first floats are the ones carry and history decide"
    ctx = context()
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, Dt, "m17hip_upload_wide_device in front of the staged block's run")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, in place behind a staged block that has not run")
        ctx.run(channels=ALL, samples=T1)
        ctx.T = T1
        _check_words(ctx.download_f32(), b.y1_all, "block 1, run behind block 2's upload")
        _run_1_is(ctx, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: m17hip_wide_channels at once ---------------------------------------------------------------------------------------------------------------
def test_retune_at_once_behind_the_staging(case, tuner_s):
    """m17hip_wide_channels never waits: it returns under the tuner.  A block already staged keeps the table it was tuned with: block 1 has the base
    table's words, which differ from table 1's on every moved channel; block 2, staged behind the call, has table 1's."""
    b, Dt = case, tuner_s
    who, src, fcw = table(1)
    assert (_u32(b.y1[who]) != _u32(b.y1_other[who])).any(axis=1).all()
    e2 = b.behind_block_1(src, fcw).block(T1, T1 + TB)
    assert (_u32(e2[who]) != _u32(b.behind_block_1().block(T1, T1 + TB)[who])).any(axis=1).all()
    ctx = context()
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_channels(rep(src), rep(fcw))
        _returned_under_the_tuner(t_s, Dt, "m17hip_wide_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the retune")
        ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), e2, "block 2, staged behind the retune")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4: m17hip_demod_reset_channels at once --------------------------------------------------------------------------------------------------------
def test_channel_reset_at_once_behind_the_staging(case, tuner_s):
    """m17hip_demod_reset_channels for a third of the first 64 channels at once behind the staging: block 1 is untouched; block 2, staged, has +0 as the
    listed channels' first output and continues every other channel (the copies of the listed channels further up in the context among them)."""
    b, Dt = case, tuner_s
    ref = b.behind_block_1()
    for c in LISTED:
        ref.carry[c] = np.zeros(2, dtype=np.float32)
    e2 = ref.block(T1, T1 + TB)
    plain = b.behind_block_1().block(T1, T1 + TB)
    rest = np.delete(np.arange(CN), LISTED)
    assert (e2[LISTED, 0] == 0).all() and (plain[LISTED, 0] != 0).all() and np.array_equal(_u32(e2[rest]), _u32(plain[rest]))
    ctx = context()
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.reset_channels(LISTED)
        _returned_under_the_tuner(t_s, Dt, "m17hip_demod_reset_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the reset")
        ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        ctx.run(channels=ALL, samples=TB)
        every = rep(plain)
        every[:CN] = e2
        _check_words(ctx.download_f32(), every, "block 2 (staged) behind the reset")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: another configuration at once ----------------------------------------------------------------------------------------------------------------
def _kept_carries(new, carries, first):
    """Block 2's expectation under a configuration that replaces block 1's: a fresh feed of `new` with the carries block 1 left."""
    plain = copy.deepcopy(new).block(0, first)
    new.carry = [c.copy() for c in carries]
    e2 = new.block(0, TB)
    assert (_u32(plain[:, 0]) != _u32(e2[:, 0])).all() and np.array_equal(_u32(plain[:, 1:]), _u32(e2[:, 1:first])), "the carries are kept, the sources start over"
    return e2


@pytest.mark.parametrize("to", ["resample", "config2"])
def test_reconfiguration_at_once_waits_for_the_resampler(case, tuner_s, to):
    """m17hip_wide_resample to another ratio (5 x 12 / 125, default taps 41 / 4001: other taps, another history, another tile) and m17hip_wide_config2 (to
    16 x 1) made at once behind the staging, before its run: wide_setup waits for the launches in flight — the call returns no earlier than the tuner can
    (its taps and histories go).  Run 1's floats and records are the old configuration's; block 2 is a fresh feed of the new one with the carries block 1
    left."""
    b, Dt = case, tuner_s
    rest = b.x[:, rows(T1):]
    if to == "resample":
        assert TB % OTHER_R[1] == 0 and rows(TB, OTHER_R) <= rest.shape[1] and tuple(t.size for t in taps(OTHER_R)) == (41, 4001)
        e2 = _kept_carries(feeds(rest, shape=OTHER_R), b.ref1.carry, OTHER_R[1])
    else:
        t1, t2 = m17hip.wide_default_taps2(*OTHER2)
        assert (t1.size, t2.size) == (129, 33) and TB * OTHER2[0] * OTHER2[1] <= rest.shape[1]
        e2 = _kept_carries(p2.PFeeds2(rest, t1, OTHER2[0], t2, OTHER2[1], SRC, FCW, GAIN), b.ref1.carry, 4)
    ctx = context()
    try:
        t_s = _stage_1(ctx, b, "device")
        t_c = time.perf_counter()
        if to == "resample":
            ctx.wide_resample(S, *OTHER_R, FMT)
        else:
            ctx.wide_config2(S, OTHER2[0], OTHER2[1], FMT)
        _waited(t_s, t_c, Dt, f"m17hip_wide_{to} before block 1's run")
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, tuned with the configuration before")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, a fresh feed of the new configuration")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_wide_resample_at_once_under_a_two_stage_block_in_flight(case, tuner2_s):
    """The reverse: the context is the two-stage tuner's (16 x 2, default taps), its block 1 staged over the same samples, and m17hip_wide_resample is the
    call made at once under tune2_kernel: it waited; run 1's floats and records are wide2_lib's; block 2 is a fresh feed of the resampler with the carries
    kept."""
    b, Dt = case, tuner2_s
    R = UNDER2[0] * UNDER2[1]
    t1, t2 = m17hip.wide_default_taps2(*UNDER2)
    assert T1 * R <= rows(T1)
    old = p2.PFeeds2(b.x, t1, UNDER2[0], t2, UNDER2[1], SRC, FCW, GAIN)
    y1 = old.block(0, T1)
    assert np.isfinite(y1).all() and not np.array_equal(_u32(y1), _u32(b.y1))
    run1 = Expect(np.ascontiguousarray(y1))
    e2 = _kept_carries(feeds(b.x[:, rows(T1):]), old.carry, U * 4)
    ctx = context(two_stage=UNDER2)
    try:
        t_s = time.perf_counter()
        ctx.upload_wide_device_async(b.at("device", 0), ALL, T1, b.pitch, GAIN)
        t_c = time.perf_counter()
        ctx.wide_resample(S, R1, U, D, FMT)
        _waited(t_s, t_c, Dt, "m17hip_wide_resample under a two-stage block")
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, (None, rep_rows(run1.run(0, T1)), rep(run1.diags)))
        _check_words(ctx.download_f32(), rep(y1), "block 1, tuned by the two-stage tuner")
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e2, "block 2, a fresh feed of the resampler")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 6: the raw buffer grows -------------------------------------------------------------------------------------------------------------------------
def test_raw_buffer_grows_behind_a_pinned_block_in_flight(case, tuner_s):
    """Block 1 from pinned memory goes through the context's raw buffer (rows of T1 / 3 x 128 samples) and its tuner reads it; its run, then an in-place
    HOST block of T1 + 192 outputs at once: the buffer is reallocated.  Block 2's words are exact, and block 1's stand behind run 1's records and
    diagnostics (the in-place block has overwritten its floats)."""
    b, Dt = case, tuner_s
    n2 = T1 + 192
    assert n2 % U == 0 and rows(T1 + n2) <= b.pitch
    e2 = b.behind_block_1().block(T1, T1 + n2)
    ctx = context(n2)
    try:
        t_s = _stage_1(ctx, b, "pinned")
        ctx.run(channels=ALL, samples=T1)
        _returned_under_the_tuner(t_s, Dt, "m17hip_demod_run in front of the block that outgrows the raw buffer")
        ctx.upload_wide(b.host(T1, T1 + n2), gain=GAIN)
        _words(ctx.download_f32(), e2, "block 2, longer than the raw buffer was")
        _run_1_is(ctx, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 7: m17hip_upload_wait at once -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pinned", "device"])
def test_upload_wait_at_once_then_the_source_overwritten(case, tuner_s, form):
    """m17hip_upload_wait blocks until the source buffer has been left: it returns no earlier than the tuner can.  The source (a copy of this case's own) is
    then overwritten and run 1's floats and records are still block 1's.  The comparisons first, the timing rule last, as in the parent."""
    import torch
    b, Dt = case, tuner_s
    mine = b.pin.clone().pin_memory() if form == "pinned" else b.dev.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = context()
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
        _run_1_is(ctx, b.idle)
        _waited(t_s, t_c, Dt, f"m17hip_upload_wait ({form})", t_r)
    finally:
        ctx.close()
        torch.cuda.synchronize()
