"""GPU tests of host calls made while the CHANNELISER is still in flight (ABI 611: m17hip_wide_raster, chan_kernel, launch_chan).  The regime is
tests/test_gpu_call_orders_wide2.py's, whose helpers and whose parents' are imported as they stand: block 1 of every case is staged and the call under test
is made at once, with nothing synchronising in between; a fresh context per case (warmed and reset: context()); a module fixture that makes the process's
first staging; floats (m17hip_download_f32) compared as uint32 words against the HOST form fed the same blocks (raster_lib.Feeds); records, m17_diag and
counts byte for byte against the float oracle on those floats.  tests/test_gpu_raster_input.py is thorough on the arithmetic; what is exercised here is the
raster's own host code underneath a queued chan_kernel: the table by source with its list of distinct bins (chan_table_words) in a turn-taking pair of its
own (rdev), rewritten on a retune AND on another channel count, the twiddle table and the histories freed and reallocated behind ev_iq, the three
configurations replacing one another and each table call refused under the others.

Shape: 2 distinct sources at decim 50, M = 192, the 1601 default taps; int16, and uint8 where marked.  Each source holds four FM transmissions from
wide_lib.wideband at -762.5, -212.5, +312.5 and +887.5 kHz: bins -61, -17, 25 and 71.  64 distinct channels, 32 per source (channel j on source j % 2):
the four transmission bins, 28 others spread over the raster with -96, 0 and 95 among them — on source 1 the last of those 28 is bin 25 once more, so that
exactly two of the 64 channels (source 1, bin 25: a transmission) are the same pair.  On a raster two channels cannot be 3 Hz apart as in the parent:
distinct bins are what makes a swap visible, and every other pair of channels differs in words (asserted, and without a GPU in tests/test_raster_input.py).

The channeliser's time goes with sources x outputs, not with channels, and a source nobody listens to returns at once: the context holds the set REP times
over, source 2 r + s the samples of distinct source s, channel 64 r + j on source 2 r + SRC[j] at BINS[j].  The host form is computed once for the two
distinct sources and every channel of the context is compared with its original.  Block 1 has T1 outputs (T1 + 1 where the count mod M has to show: see
test_run_then_block_2_in_place_at_once), the blocks behind it 384.

The premise is the parent's: a module fixture measures D on a throwaway context (the smallest of three single-launch readings of timing index 11 from
in-place device blocks of T1 outputs); t_s just before the staging call, t_c just before the call under test, t_r when it returns.  A call that must not
wait has t_r - t_s < 0.5 D; one that must wait was made with t_c - t_s < 0.5 D and returned with t_r - t_s >= 0.5 D.  A case whose premise fails FAILS.
Timing is off inside the cases.  (REP, T1) is the smallest of {64, 128} x {4800, 9600, 19200} — by sources x outputs, the fewer sources first — at which D
is at least eight times the longest t_r - t_s of the calls that do not wait, measured once on the MI355X with the product build, with the pinned and the
device copy of the sources at or below 512 MB each: (64, 9600).  T1 = 4800 is no candidate for a reason of its own: 2.5 frames hold no record of most
transmissions (of 24 generator seeds none gave more than two of the nine transmission channels a record), and the transmission bins must yield records.  At
(64, 9600) D is 2.31 - 2.44 ms (uint8 the shorter) and the longest such interval 0.18 ms, a factor 12.9; the sources are 501 MB; (128, 9600) and
(64, 19200) would be 1.0 GB.  NOTES.md has the readings and the intervals.
"""
import copy
import ctypes as C
import time

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol
import raster_lib as rl
import test_gpu_call_orders_formats as par
import test_gpu_call_orders_wide as pw
import test_gpu_call_orders_wide2 as p2
import wide_lib as wl
from test_gpu_call_orders_formats import CN, DIAG_STREAM, THREADS, Expect, _check_diag, _check_records, _check_words, _in_flight, _u32
from test_gpu_call_orders_wide2 import NOT_A_PASS, PFeeds2, pw_dev   # noqa: F401

pytestmark = pytest.mark.gpu

ESTATE = -4
S, R, M = 2, 50, 192
REP = 64                     # times the 64 channels and the 2 sources are held: 128 sources, 4096 channels (chosen by the rule above)
T1 = 9600                    # outputs of block 1, whose channeliser is in flight (likewise)
TB = 384                     # outputs of the blocks behind it
TOTAL = 2 * T1 + TB          # outputs the sources hold: block 1, then T1 + 192 for the block that outgrows the raw buffer, or up to three of TB
ALL, NS = CN * REP, S * REP
T0F = p2.T0F                 # samples of a float run 0 that keeps the main stream busy
OFFSETS = p2.OFFSETS
TX_BINS = (-61, -17, 25, 71)
assert all(12500.0 * b == f for b, f in zip(TX_BINS, OFFSETS))
PER_SOURCE = pw.PER_SOURCE
FMTS, AMPLITUDE, SIGMA, SB, GAIN = pw.FMTS, pw.AMPLITUDE, pw.SIGMA, pw.SB, pw.GAIN
LISTED = p2.LISTED
SRC = pw.SRC                 # channel j listens to source j % 2
_OTHERS = [-96, 0, 95] + list(range(-93, 76, 7))
assert len(_OTHERS) == 28 and len(set(_OTHERS) | set(TX_BINS)) == 32 and all(-96 <= b <= 95 for b in _OTHERS)
_ORDER = np.random.default_rng(611).permutation(32)
_PER = [np.array(list(TX_BINS) + _OTHERS)[_ORDER], np.array(list(TX_BINS) + _OTHERS[:-1] + [TX_BINS[2]])[_ORDER]]
BINS = np.array([_PER[j % S][j // S] for j in range(CN)], dtype=np.int64)
PAIR = tuple(int(j) for j in np.flatnonzero((SRC == 1) & (BINS == TX_BINS[2])))      # the two channels on one (source, bin)
TX_CHANNELS = [int(j) for j in range(CN) if BINS[j] in TX_BINS]
assert len(PAIR) == 2 and len(TX_CHANNELS) == 9 and len({(int(s), int(b)) for s, b in zip(SRC, BINS)}) == CN - 1
assert T1 % 192 == 0 and TB % 192 == 0 and ((T1 + 1) * R) % M != 0
TAPS = None                  # (the default taps: from the library, on first use)
# the configurations that replace decim 50 / 192 bins
RASTER_DECIM = 40            # m17hip_wide_raster with the same bins: 1281 default taps, the table kept
RASTER_BINS = 128            # ... with other bins: the table starts over
OTHER2, OTHER1 = p2.OTHER2, p2.OTHER1


def taps():
    global TAPS
    if TAPS is None:
        TAPS = m17hip.wide_raster_default_taps(R)
        assert TAPS.size == 1601
    return TAPS


def table(k):
    """Table k = 1, 2, 3 beside the base table: another quarter of the channels on the OTHER source — first[], the pairs and the list of distinct bins all
    change — by turns at a bin the new source's listeners already have (several channels on one bin) and three bins beside their own (a bin nobody had)."""
    who = np.arange(k, CN, 4)
    src, bins = SRC.copy(), BINS.copy()
    src[who] = 1 - src[who]
    for i, c in enumerate(who):
        bins[c] = BINS[(c + 1 + 2 * k) % CN] if i % 2 == 0 else (BINS[c] + 3 if BINS[c] + 3 <= 95 else BINS[c] - 3)
    return who, src, bins


def rep(a):
    """Per-channel rows of the 64 distinct channels -> of all the context's channels."""
    a = np.asarray(a)
    return np.tile(a, (REP,) + (1,) * (a.ndim - 1))


def rep_src(src):
    """The sources of the 64 distinct channels -> of all the context's channels: copy r listens to sources 2 r and 2 r + 1."""
    return (np.asarray(src, dtype=np.int64)[None, :] + S * np.arange(REP)[:, None]).reshape(-1)


def rep_rows(rows):
    out = []
    for c in range(ALL):
        q = rows[c % CN].copy()
        q["channel"] = c
        out.append(q)
    return np.concatenate(out)


def feeds(x, src=SRC, bins=BINS, decim=R, bins_of=M, h=None):
    return rl.Feeds(x, taps() if h is None else h, decim, bins_of, src, bins, GAIN)


def sources(fmt, total=None, seed=20261022):
    total = TOTAL if total is None else total
    p = ol.gen_params(seed=seed, kind=-1, n_frames=max(total // 1920 - 3, 1), lead_in=48, total=total)
    bb = ol.generate_batch(p, S * PER_SOURCE, total, threads=THREADS)
    x = np.stack([wl.wideband(bb[PER_SOURCE * s: PER_SOURCE * (s + 1)], OFFSETS, R, amplitude=AMPLITUDE[fmt], sigma=SIGMA[fmt], seed=s + 1, fmt=fmt) for s in range(S)])
    x.setflags(write=False)
    return x


def one_pair_alike(y):
    """The premise that makes a swap of two channels visible: the two channels of PAIR have the same words, every other pair of channels differs."""
    w = _u32(y)
    alike = [(a, b) for a in range(CN) for b in range(a + 1, CN) if np.array_equal(w[a], w[b])]
    assert alike == [PAIR], alike


def moved_differ(a, b, who):
    assert (_u32(a[who]) != _u32(b[who])).any(axis=1).all()


class Case:
    """The sources of one format in host memory and — REP times over — in pinned and device memory; block 1's floats under the base table (y1) and under
    table 1 (y1_other), the feed's state behind block 1 (ref1: deep-copied by whoever continues it), the same for a block 1 of T1 + 1 outputs (y1p, ref1p),
    and the float oracle's records for run 1 alone and behind a float run 0."""

    def __init__(self, fmt, x0f):
        import torch
        t0 = time.perf_counter()
        self.fmt, self.sb = fmt, SB[fmt]
        self.x = sources(fmt)
        t1 = time.perf_counter()
        ref = feeds(self.x)
        self.y1 = ref.block(0, T1)
        self.ref1 = ref
        refp = feeds(self.x)
        self.y1p = refp.block(0, T1 + 1)
        self.ref1p = refp
        assert np.array_equal(_u32(self.y1), _u32(self.y1p[:, :T1]))
        _, src, bins = table(1)
        self.y1_other = feeds(self.x, src, bins).block(0, T1)
        assert np.isfinite(self.y1p).all()
        one_pair_alike(self.y1)
        for a in (self.y1, self.y1p, self.y1_other):
            a.setflags(write=False)
        t2 = time.perf_counter()
        self.pitch = TOTAL * R
        every = torch.from_numpy(np.array(self.x)).repeat(REP, 1, 1)
        assert every.shape[0] == NS and every.numel() * every.element_size() <= 512 * 10 ** 6
        self.pin = every.pin_memory()
        self.dev = every.cuda()
        torch.cuda.synchronize()
        del every
        t3 = time.perf_counter()
        idle = Expect(np.ascontiguousarray(self.y1))
        self.idle = (None, rep_rows(idle.run(0, T1)), rep(idle.diags))
        assert all(idle.run(0, T1)[c].size > 0 for c in TX_CHANNELS), "every channel on a transmission's bin yields records"
        idlep = Expect(np.ascontiguousarray(self.y1p))
        self.idlep = (None, rep_rows(idlep.run(0, T1 + 1)), rep(idlep.diags))
        busy = Expect(np.concatenate([x0f, self.y1], axis=1))
        self.busy = (rep_rows(busy.run(0, T0F)), rep_rows(busy.run(T0F, T0F + T1)), rep(busy.diags))
        assert self.busy[0].size > ALL and self.busy[1].size > 0, "run 1 yields records"
        self.y1_all, self.y1p_all = rep(self.y1), rep(self.y1p)
        for a in (self.y1_all, self.y1p_all):
            a.setflags(write=False)
        t4 = time.perf_counter()
        print(f"[raster] fixture ({'i16' if fmt == wl.IQ_I16 else 'u8'}): sources {t1 - t0:.2f} s, host form on two sources {t2 - t1:.2f} s, "
              f"pinning and device copy {t3 - t2:.2f} s, float oracle {t4 - t3:.2f} s")

    def at(self, where, a, rate=R):
        """The pointer to the first sample of output a (at `rate` samples an output) in the pinned or the device copy."""
        base = self.pin.data_ptr() if where == "pinned" else self.dev.data_ptr()
        return base + a * rate * self.sb

    def host(self, a, b):
        """Outputs [a, b) of every source of the context, in host memory."""
        return np.ascontiguousarray(np.tile(self.x[:, a * R: b * R], (REP, 1, 1)))

    def behind_block_1(self, src=None, bins=None, plus=False):
        r = copy.deepcopy(self.ref1p if plus else self.ref1)
        if src is not None:
            r.src, r.bins = list(src), list(bins)
        return r


_SILENCE = {}


def _configure(ctx, fmt):
    ctx.wide_raster(NS, R, M, fmt)
    ctx.wide_raster_channels(rep_src(SRC), rep(BINS))


def context(fmt, maxT=T1, raw_from=None, raw_n=T1):
    """A fresh context under the base table that has made its first in-place block, its first staging and two runs, and was then reset (the parent's
    context(): the first staging of a context allocates its second slab pair, the second float slab and the copy stream and publishes the table).  With
    `raw_from` (a Case) the staging is that case's block 1 (raw_n outputs) from PINNED memory: the raw buffer of the host forms — here sources x T1 x 50 samples, not the
    parent's two rows — is allocated in the warm-up, not inside the interval a case measures.  m17hip_demod_reset then starts the stream and the sources'
    feeds over: what a case sees is a fresh stream."""
    import torch
    if fmt not in _SILENCE:
        _SILENCE[fmt] = torch.zeros((NS, TB * R, 2), dtype=torch.int16 if fmt == wl.IQ_I16 else torch.uint8, device="cuda")
        torch.cuda.synchronize()
    quiet = _SILENCE[fmt].data_ptr()
    ctx = m17hip.Context(ALL, maxT)
    try:
        _configure(ctx, fmt)
        ctx.upload_wide_device(quiet, ALL, TB, TB * R)
        ctx.run()
        if raw_from is None:
            ctx.upload_wide_device_async(quiet, ALL, TB, TB * R)
            ctx.run(channels=ALL, samples=TB)
        else:
            ctx.upload_wide_async(raw_from.at("pinned", 0), ALL, raw_n, raw_from.pitch, GAIN)
            ctx.run(channels=ALL, samples=raw_n)
        ctx.frames()
        ctx.upload_wait()
        ctx.reset()
    except Exception:
        ctx.close()
        raise
    return ctx


def _frames_once(ctx):
    """m17hip_frames_fetch ONCE with room for every record of every channel (the parent's, sized for this module's channels)."""
    recs = np.zeros(ALL * par._rec_cap(T0F + T1 + 1), dtype=m17hip.FRAME_REC)
    got = C.c_uint64(0)
    ctx._chk(ctx.lib.m17hip_frames_fetch(ctx.h, m17hip._ptr(recs), C.c_uint64(recs.size), C.byref(got)))
    return recs[: got.value]


def _words(got, exp64, what):
    _check_words(got, rep(exp64), what)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def first_staging_of_the_process():
    """The parent modules' throwaway staging, and under the raster one block in place, one host block, one retune and one staged pinned block; then the
    same under the two-stage tuner: the copy stream, the pinned staging of both channel tables and their device copies have been allocated once in this
    process before any case is timed."""
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
    w = np.zeros((NS, TB * R, 2), dtype=np.int16)
    wpin = torch.from_numpy(w.copy()).pin_memory()
    ctx = context(wl.IQ_I16, TB)
    try:
        ctx.upload_wide(w)
        ctx.run()
        ctx.wide_raster_channels(rep_src(SRC[::-1].copy()), rep(BINS))
        ctx.upload_wide_async(wpin.data_ptr(), ALL, TB, TB * R)
        ctx.run(channels=ALL, samples=TB)
        ctx.frames()
        ctx.upload_wait()
        ctx.wide_config2(NS, OTHER2[0], OTHER2[1], wl.IQ_I16)
        ctx.wide_channels(rep_src(SRC), rep(BINS))
        ctx.upload_wide_device(_SILENCE[wl.IQ_I16].data_ptr(), ALL, TB, TB * R)
        ctx.run()
        ctx.wide_channels(rep_src(SRC[::-1].copy()), rep(BINS))
        ctx.upload_wide_device_async(_SILENCE[wl.IQ_I16].data_ptr(), ALL, TB, TB * R)
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


def _three_readings(ctx, kernel, block):
    ctx.timing(True)
    reads = []
    for _ in range(3):
        ctx.timing_reset()
        block()
        ms, launches = ctx.timing_get(kernel)
        assert launches == 1 and ms > 0
        reads.append(ms)
    ctx.timing(False)
    return reads


@pytest.fixture(scope="module")
def chan_s(cases, first_staging_of_the_process):
    """D per format, in seconds: the smallest of three single-launch readings of timing index 11 on a throwaway context."""
    out = {}
    for name, b in cases.items():
        ctx = context(b.fmt)
        try:
            reads = _three_readings(ctx, "channelise", lambda: ctx.upload_wide_device(b.at("device", 0), ALL, T1, b.pitch, GAIN))
        finally:
            ctx.close()
        out[name] = 1e-3 * min(reads)
        print(f"[raster] D ({name}, {NS} sources x {T1} outputs): {min(reads):.3f} ms (readings {', '.join(f'{r:.3f}' for r in reads)})")
    return out


def _fcw16():
    """A frequency word per distinct channel for the tuners that take over at 16 x: the channel's bin as a frequency, taken at that rate."""
    return np.array([m17hip.wide_fcw(12500.0 * b / 4.0, 16) for b in BINS], dtype=np.int64)


@pytest.fixture(scope="module")
def tuner2_s(cases, first_staging_of_the_process):
    """The two-stage tuner's time (16 x 1, timing index 10) for T1 outputs of every channel, measured the same way: what m17hip_wide_raster waits for when
    it takes over from m17hip_wide_config2 behind a staged block."""
    b = cases["i16"]
    ctx = context(b.fmt)
    try:
        ctx.wide_config2(NS, OTHER2[0], OTHER2[1], b.fmt)
        ctx.wide_channels(rep_src(SRC), rep(_fcw16()))
        reads = _three_readings(ctx, "tune2", lambda: ctx.upload_wide_device(b.at("device", 0), ALL, T1, b.pitch, GAIN))
    finally:
        ctx.close()
    print(f"[raster] D2 (tune2_kernel at 16 x 1, {ALL} channels x {T1} outputs): {min(reads):.3f} ms (readings {', '.join(f'{r:.3f}' for r in reads)})")
    return 1e-3 * min(reads)


# ---- the steps of a case -------------------------------------------------------------------------------------------------------------------------
def _stage_1(ctx, b, form, n=T1):
    """Block 1, staged: its channeliser runs on the copy stream.  Returns t_s."""
    t_s = time.perf_counter()
    if form == "pinned":
        ctx.upload_wide_async(b.at("pinned", 0), ALL, n, b.pitch, GAIN)
    else:
        ctx.upload_wide_device_async(b.at("device", 0), ALL, n, b.pitch, GAIN)
    return t_s


def _made_under(t_s, D, what, t_c=None):
    """The premise of a call made at t_c (default: now): block 1's channeliser, which cannot end before t_s + D, had more than half of its time left."""
    t_c = time.perf_counter() if t_c is None else t_c
    print(f"[raster] {what}: made {1e3 * (t_c - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_c - t_s < 0.5 * D, f"{what} was made {1e3 * (t_c - t_s):.3f} ms after the staging call began, the channeliser takes {1e3 * D:.3f} ms: it may have " \
                                f"finished on the device before the call under test was made: {NOT_A_PASS}"
    return t_c


def _returned_under(t_s, D, what):
    """A call that must not wait has returned: t_r - t_s < 0.5 D (which says as well that it was made under the channeliser)."""
    t_r = time.perf_counter()
    print(f"[raster] {what}: returned {1e3 * (t_r - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_r - t_s < 0.5 * D, f"{what} returned {1e3 * (t_r - t_s):.3f} ms after the staging call began, the channeliser takes {1e3 * D:.3f} ms: either it waited, " \
                                f"or the channeliser may have finished on the device before the call under test was made: {NOT_A_PASS}"


def _waited(t_s, t_c, D, what, t_r=None):
    """A call that must wait for the launches in flight has returned (at t_r; default: now): it was made under the kernel and came back no earlier than
    half of D."""
    t_r = time.perf_counter() if t_r is None else t_r
    print(f"[raster] {what}: made {1e3 * (t_c - t_s):.3f} ms, returned {1e3 * (t_r - t_s):.3f} ms after the staging call began (D = {1e3 * D:.3f} ms)")
    assert t_c - t_s < 0.5 * D, f"{what} was made {1e3 * (t_c - t_s):.3f} ms after the staging call began, the kernel takes {1e3 * D:.3f} ms: {NOT_A_PASS}"
    assert t_r - t_s >= 0.5 * D, f"{what} returned {1e3 * (t_r - t_s):.3f} ms after the staging call began: it did not wait for a kernel that takes {1e3 * D:.3f} ms"


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


def _block_2(ctx, b, a=T1, n=TB):
    """The block behind block 1, in place on the main stream from device memory."""
    ctx.upload_wide_device(b.at("device", a), ALL, n, b.pitch, GAIN)


# ---- 1: m17hip_demod_run at once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,form,main", [("i16", "pinned", "idle"), ("i16", "pinned", "run_0"), ("i16", "device", "idle"), ("i16", "device", "run_0"),
                                           ("u8", "device", "idle"), ("u8", "device", "run_0")])
def test_run_at_once_behind_the_staging(cases, chan_s, run0_floats, fmt, form, main):
    """m17hip_demod_run returns under the channeliser; what it queued waited for the staging: run 1's records and diagnostics are the float oracle's on
    block 1's floats — the only check there is that the run waited — and the floats, fetched afterwards, the host form's.  With the main stream idle, and
    with a float run 0 of 24 000 samples in flight on it (asserted)."""
    b, D = cases[fmt], chan_s[fmt]
    busy = main == "run_0"
    ctx = context(b.fmt, T0F if busy else T1, raw_from=b if form == "pinned" else None)
    try:
        if busy:
            ctx.upload_device(run0_floats[1].data_ptr(), ALL, T0F, dtype=np.float32)
            ctx.run()
            _in_flight(ctx)
        t_s = _stage_1(ctx, b, form)
        ctx.run(channels=ALL, samples=T1)
        _returned_under(t_s, D, f"m17hip_demod_run ({form}, {main})")
        _run_1_is(ctx, b, b.busy if busy else b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "the floats run 1 read")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 2: run, then block 2 in place on the main stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("form", ["host", "device"])
def test_run_then_block_2_in_place_at_once(cases, chan_s, form, fmt):
    """Block 1 staged (from pinned memory in front of a host block, from device memory in front of a device block), its run, and block 2 in place on the
    MAIN stream at once: its words continue block 1 — the sources' histories, the count mod M and the channels' carries crossed from the copy stream
    through ev_iq alone.  Block 1 has T1 + 1 outputs here: T1 x 50 is a multiple of 192 for every T1 this module may take, and (T1 + 1) x 50 mod 192 = 50,
    so a count that did not cross shows in block 2's words (asserted against a feed that has lost it)."""
    b, D = cases[fmt], chan_s[fmt]
    n1 = T1 + 1
    e2 = b.behind_block_1(plus=True).block(n1, n1 + TB)
    fresh = feeds(b.x[:, n1 * R:]).block(0, 4)
    assert (_u32(fresh[:, 0]) != _u32(e2[:, 0])).all() and (_u32(fresh[:, 1:]) != _u32(e2[:, 1:4])).any(), "block 2's first floats are the ones carry and history decide"
    lost = b.behind_block_1(plus=True)
    for t in lost.per_source:
        t.count = 0
    assert lost.per_source[0].count % M != b.ref1p.per_source[0].count % M
    assert (_u32(lost.block(n1, n1 + TB)) != _u32(e2)).any(axis=1)[[c for c in range(CN) if (BINS[c] * (n1 * R)) % M != 0]].all(), "the count mod M decides block 2's words"
    ctx = context(b.fmt, n1, raw_from=b if form == "host" else None, raw_n=n1)
    try:
        t_s = _stage_1(ctx, b, "pinned" if form == "host" else "device", n1)
        ctx.run(channels=ALL, samples=n1)
        _returned_under(t_s, D, f"m17hip_demod_run in front of an in-place block ({form})")
        if form == "host":
            ctx.upload_wide(b.host(n1, n1 + TB), gain=GAIN)
        else:
            _block_2(ctx, b, n1)
        _words(ctx.download_f32(), e2, "block 2, in place behind a staged block")
        _run_1_is(ctx, b, b.idlep)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: block 2 in place before block 1's run ------------------------------------------------------------------------------------------------------
def test_block_2_in_place_at_once_before_block_1s_run(cases, chan_s):
    """Block 2 in place on the main stream at once behind the staging, BEFORE block 1's run: nothing but ev_iq stands between the two channelisers.
    Blocks continue one another in call order: block 2's words continue block 1; run 1 then reads the staged block 1, untouched."""
    b, D = cases["i16"], chan_s["i16"]
    e2 = b.behind_block_1().block(T1, T1 + TB)
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under(t_s, D, "m17hip_upload_wide_device in front of the staged block's run")
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, in place behind a staged block that has not run")
        ctx.run(channels=ALL, samples=T1)
        ctx.T = T1
        _check_words(ctx.download_f32(), b.y1_all, "block 1, run behind block 2's upload")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4, 5: m17hip_wide_raster_channels at once -----------------------------------------------------------------------------------------------------
def test_retune_at_once_behind_the_staging(cases, chan_s):
    """m17hip_wide_raster_channels "never waits for anything in flight": it returns under the channeliser.  "A block already staged keeps the table it was
    tuned with": block 1 has the base table's words, which differ from table 1's on every moved channel; block 2, in place, has table 1's."""
    b, D = cases["i16"], chan_s["i16"]
    who, src, bins = table(1)
    moved_differ(b.y1, b.y1_other, who)
    e2 = b.behind_block_1(src, bins).block(T1, T1 + TB)
    moved_differ(e2, b.behind_block_1().block(T1, T1 + TB), who)
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_raster_channels(rep_src(src), rep(bins))
        _returned_under(t_s, D, "m17hip_wide_raster_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the retune")
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, in place behind the retune")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_retunes_back_to_back_each_table_copy_rewritten_under_channelisers(cases, chan_s):
    """Two retunes back to back behind the staging, the run, a staged block 2 (it publishes table 2 into the copy of rdev block 1's channeliser does NOT
    read), a third retune, the run, a staged block 3 (table 3 goes into the copy block 1 read): each copy is rewritten while launches that read it were
    queued.  Block 1 has the base table's words, block 2 table 2's, block 3 table 3's."""
    b, D = cases["i16"], chan_s["i16"]
    tables = [table(k) for k in (1, 2, 3)]
    ref = b.behind_block_1(*tables[1][1:])
    e2 = ref.block(T1, T1 + TB)
    ref.src, ref.bins = list(tables[2][1]), list(tables[2][2])
    e3 = ref.block(T1 + TB, T1 + 2 * TB)
    moved_differ(e2, b.behind_block_1(*tables[0][1:]).block(T1, T1 + TB), tables[1][0])   # table 2, not table 1
    ctx = context(b.fmt, raw_from=b)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_raster_channels(rep_src(tables[0][1]), rep(tables[0][2]))
        ctx.wide_raster_channels(rep_src(tables[1][1]), rep(tables[1][2]))
        ctx.run(channels=ALL, samples=T1)
        _returned_under(t_s, D, "two retunes back to back and m17hip_demod_run")
        ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)   # (queued behind block 1's channeliser: stream order)
        ctx.wide_raster_channels(rep_src(tables[2][1]), rep(tables[2][2]))
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


# ---- 6: another channel count, nothing retuned -----------------------------------------------------------------------------------------------------
def test_channel_count_shrinks_and_grows_with_nothing_retuned(cases, chan_s):
    """launch_chan rewrites the table on a condition the tuners do not have: a block with another channel count republishes it although nobody retuned.
    Block 1 staged with every channel, its run, block 2 at once with the first 64 (the first copy of the distinct set) — a continued stream keeps its
    channel count from run to run, so block 2 is tuned in place and is not run: its table goes into the other copy of rdev under block 1's channeliser —,
    block 3, in place as well, with all again.  Each block's listed rows are the host form's.  Block 2 is written into the slab run 1 read, behind the run: run 1's
    records and diagnostics stand for block 1, and what block 2 does not cover of it — the rows above 64, and the first 64 from output 384 on — is
    untouched.  A block of 64 channels carries the sources' histories and the count on and leaves the carries of the channels above alone: in block 3
    those continue block 1's last z."""
    b, D = cases["i16"], chan_s["i16"]
    ref = b.behind_block_1()
    kept = ref.carry.copy()
    e2 = ref.block(T1, T1 + TB)
    above = copy.deepcopy(ref)
    above.carry = kept
    e3, e3_above = ref.block(T1 + TB, T1 + 2 * TB), above.block(T1 + TB, T1 + 2 * TB)
    assert (_u32(e3[:, 0]) != _u32(e3_above[:, 0])).all() and np.array_equal(_u32(e3[:, 1:]), _u32(e3_above[:, 1:]))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.run(channels=ALL, samples=T1)
        _made_under(t_s, D, "m17hip_upload_wide_device with 64 channels")
        ctx.upload_wide_device(b.at("device", T1), CN, TB, b.pitch, GAIN)
        _check_words(ctx.download_f32(), e2, "block 2, the first 64 channels")
        _run_1_is(ctx, b, b.idle)
        ctx.C, ctx.T = ALL, T1
        left = np.array(b.y1_all)
        left[:CN, :TB] = e2
        _check_words(ctx.download_f32(), left, "block 1 around block 2, a republication queued behind it")
        ctx.upload_wide_device(b.at("device", T1 + TB), ALL, TB, b.pitch, GAIN)
        every = rep(e3_above)
        every[:CN] = e3
        _check_words(ctx.download_f32(), every, "block 3, every channel again")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_channel_count_grows_first_with_nothing_retuned(cases, chan_s):
    """The order growing first: a block of 384 outputs with the first 64 channels in place (only two sources have listeners: its channeliser is short and
    is no premise), then at once the long block with ALL channels, staged, and its run: the grown table is published for a launch that is then in flight
    — the table of 64 would be valid for it and merely leave the rows above unwritten.  Every row of the long block is the host form's; the rows above 64
    start from a zero carry behind the first block's histories and count."""
    b, D = cases["i16"], chan_s["i16"]
    ref = feeds(b.x)
    e1 = ref.block(0, TB)
    assert np.array_equal(_u32(e1), _u32(b.y1[:, :TB]))
    above = copy.deepcopy(ref)
    above.carry[:] = 0
    e2, e2_above = ref.block(TB, TB + T1), above.block(TB, TB + T1)
    assert (e2_above[:, 0] == 0).all() and (e2[:, 0] != 0).all() and np.array_equal(_u32(e2[:, 1:]), _u32(e2_above[:, 1:]))
    ctx = context(b.fmt)
    try:
        ctx.upload_wide_device(b.at("device", 0), CN, TB, b.pitch, GAIN)
        _check_words(ctx.download_f32(), e1, "block 1, the first 64 channels")
        t_s = time.perf_counter()
        ctx.upload_wide_device_async(b.at("device", TB), ALL, T1, b.pitch, GAIN)
        ctx.run(channels=ALL, samples=T1)
        _returned_under(t_s, D, "a staged block of every channel behind one of 64, and m17hip_demod_run")
        every = rep(e2_above)
        every[:CN] = e2
        _check_words(ctx.download_f32(), every, "block 2, every channel behind a block of 64")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 7, 8: resets at once --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", ["in_place", "staged"])
def test_channel_reset_at_once_behind_the_staging(cases, chan_s, second):
    """m17hip_demod_reset_channels for a third of the first 64 channels at once behind the staging: the carries are zeroed behind block 1's channeliser, on
    its stream.  Block 1 is untouched; block 2 — in place on the main stream, or staged — has +0 as the listed channels' first output and continues every
    other channel (the copies of the listed channels further up in the context among them)."""
    b, D = cases["i16"], chan_s["i16"]
    ref = b.behind_block_1()
    ref.carry[LISTED] = 0
    e2 = ref.block(T1, T1 + TB)
    plain = b.behind_block_1().block(T1, T1 + TB)
    rest = np.delete(np.arange(CN), LISTED)
    assert (e2[LISTED, 0] == 0).all() and (plain[LISTED, 0] != 0).all() and np.array_equal(_u32(e2[rest]), _u32(plain[rest]))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.reset_channels(LISTED)
        _returned_under(t_s, D, "m17hip_demod_reset_channels")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, staged before the reset")
        if second == "in_place":
            _block_2(ctx, b)
        else:
            ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)
            ctx.run(channels=ALL, samples=TB)
        every = rep(plain)
        every[:CN] = e2
        _check_words(ctx.download_f32(), every, f"block 2 ({second}) behind the reset")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_reset_at_once_behind_the_run(cases, chan_s):
    """m17hip_demod_reset at once behind block 1's run: block 2 starts from zero histories, a zero count and zero carries — a fresh host form."""
    b, D = cases["i16"], chan_s["i16"]
    e2 = feeds(b.x[:, T1 * R:]).block(0, TB)
    assert not np.array_equal(_u32(e2), _u32(b.behind_block_1().block(T1, T1 + TB)))
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.run(channels=ALL, samples=T1)
        _made_under(t_s, D, "m17hip_demod_reset")
        ctx.reset()
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2 behind m17hip_demod_reset")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 9: another configuration at once --------------------------------------------------------------------------------------------------------------
def _reconfigure(ctx, b, to):
    """(the call under test, what follows it before block 2, block 2's expectation, the new feed): a fresh feed of the new configuration over the samples
    behind block 1 with the carries kept.  raster_decim keeps the table (the bins are the same); raster_bins starts it over (every channel on source 0, bin
    0: a bin of 192 is none of 128), and so do the tuners, whose table is then written with m17hip_wide_channels."""
    rest = b.x[:, T1 * R:]
    after = lambda: None
    if to == "raster_decim":
        new = feeds(rest, decim=RASTER_DECIM, h=m17hip.wide_raster_default_taps(RASTER_DECIM))
        call = lambda: ctx.wide_raster(NS, RASTER_DECIM, M, b.fmt)
        rate = RASTER_DECIM
    elif to == "raster_bins":
        new = feeds(rest, [0] * CN, [0] * CN, bins_of=RASTER_BINS)
        call = lambda: ctx.wide_raster(NS, R, RASTER_BINS, b.fmt)
        rate = R
    elif to == "config2":
        t1, t2 = m17hip.wide_default_taps2(*OTHER2)
        new = PFeeds2(rest, t1, OTHER2[0], t2, OTHER2[1], SRC, _fcw16(), GAIN)
        call = lambda: ctx.wide_config2(NS, OTHER2[0], OTHER2[1], b.fmt)
        after = lambda: ctx.wide_channels(rep_src(SRC), rep(_fcw16()))
        rate = OTHER2[0] * OTHER2[1]
    else:
        h = wl.hamming_taps(OTHER1[1])
        new = pw.PFeeds(rest, h, SRC, _fcw16(), OTHER1[0], GAIN)
        call = lambda: ctx.wide_config(NS, OTHER1[0], b.fmt, h)
        after = lambda: ctx.wide_channels(rep_src(SRC), rep(_fcw16()))
        rate = OTHER1[0]
    plain = copy.deepcopy(new).block(0, 4)
    if isinstance(new, rl.Feeds):
        new.carry[:] = b.ref1.carry
    else:
        new.carry = [c.copy() for c in b.ref1.carry]
    e2 = new.block(0, TB)
    assert (_u32(plain[:, 0]) != _u32(e2[:, 0])).all() and np.array_equal(_u32(plain[:, 1:]), _u32(e2[:, 1:4])), "the carries are kept, the sources start over"
    assert TB * rate <= (TOTAL - T1) * R
    return call, after, e2, new


RECONFIGURATIONS = ["raster_decim", "raster_bins", "config2", "config"]


@pytest.mark.parametrize("where", ["before_its_run", "behind_its_run"])
@pytest.mark.parametrize("to", RECONFIGURATIONS)
def test_reconfiguration_at_once_waits_for_the_channeliser(cases, chan_s, to, where):
    """m17hip_wide_raster (another decimation with the same bins; other bins), m17hip_wide_config2 and m17hip_wide_config "wait for the launches in
    flight": made at once behind the staging BEFORE its run, and at once behind its run, the call returns no earlier than the channeliser can — the
    histories, the taps and the twiddle table go.  Run 1's floats and records are the old configuration's; block 2 is a fresh feed of the new one with the
    carries block 1 left."""
    b, D = cases["i16"], chan_s["i16"]
    ctx = context(b.fmt)
    try:
        call, after, e2, _ = _reconfigure(ctx, b, to)
        t_s = _stage_1(ctx, b, "device")
        if where == "behind_its_run":
            ctx.run(channels=ALL, samples=T1)
        t_c = time.perf_counter()
        call()
        _waited(t_s, t_c, D, f"{to} {where}")
        after()
        if where == "before_its_run":
            ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "block 1, channelised with the configuration before")
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, a fresh feed of the new configuration")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_raster_again_at_once_behind_a_staged_block_of_the_two_stage_tuner(cases, chan_s, tuner2_s):
    """m17hip_wide_config2 behind block 1's run (it waits for the channeliser), one block of the two-stage tuner in place, then a block of T1 outputs of
    it STAGED and m17hip_wide_raster at once: it waits for tune2_kernel, and the twiddle table, released under the tuner, is allocated afresh.  The staged
    block has the tuner's words; the block behind is the raster's from a fresh feed and a fresh table (source 0, bin 0) with the carries the tuner left."""
    b, D, D2 = cases["i16"], chan_s["i16"], tuner2_s
    step = OTHER2[0] * OTHER2[1]
    assert (T1 * step) % R == 0 and (TB + T1) * step + TB * R <= (TOTAL - T1) * R
    ctx = context(b.fmt)
    try:
        call, after, e2, two = _reconfigure(ctx, b, "config2")
        e3 = two.block(TB, TB + T1)
        a4 = T1 * R + (TB + T1) * step                      # (in samples of the sources)
        back = feeds(b.x[:, a4:], [0] * CN, [0] * CN)
        back.carry[:] = np.stack(two.carry)
        e4 = back.block(0, TB)
        t_s = _stage_1(ctx, b, "device")
        ctx.run(channels=ALL, samples=T1)
        t_c = time.perf_counter()
        call()
        _waited(t_s, t_c, D, "m17hip_wide_config2 behind block 1's run")
        after()
        _run_1_is(ctx, b, b.idle)
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, the two-stage tuner's")
        at3 = b.dev.data_ptr() + (T1 * R + TB * step) * b.sb
        t_s = time.perf_counter()
        ctx.upload_wide_device_async(at3, ALL, T1, b.pitch, GAIN)
        t_c = time.perf_counter()
        ctx.wide_raster(NS, R, M, b.fmt)
        _waited(t_s, t_c, D2, "m17hip_wide_raster behind a staged block of the two-stage tuner")
        ctx.run(channels=ALL, samples=T1)
        _words(ctx.download_f32(), e3, "block 3, staged under the two-stage tuner")
        ctx.upload_wide_device(b.dev.data_ptr() + a4 * b.sb, ALL, TB, b.pitch, GAIN)
        _words(ctx.download_f32(), e4, "block 4, the raster again: a fresh table, the tuner's carries")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 10: the raw buffer grows ----------------------------------------------------------------------------------------------------------------------
def test_raw_buffer_grows_behind_a_pinned_block_in_flight(cases, chan_s):
    """Block 1 from pinned memory goes through the context's raw buffer (sized for T1 outputs of every source) and its channeliser reads it; its run, then
    an in-place HOST block of T1 + 192 outputs at once: the buffer is reallocated.  Block 2's words are exact, and block 1's stand behind run 1's records
    and diagnostics (the in-place block has overwritten its floats)."""
    b, D = cases["i16"], chan_s["i16"]
    n2 = T1 + 192
    e2 = b.behind_block_1().block(T1, T1 + n2)
    x2 = b.host(T1, T1 + n2)
    ctx = context(b.fmt, n2, raw_from=b)
    try:
        t_s = _stage_1(ctx, b, "pinned")
        ctx.run(channels=ALL, samples=T1)
        _returned_under(t_s, D, "m17hip_demod_run in front of the block that outgrows the raw buffer")
        ctx.upload_wide(x2, gain=GAIN)
        _words(ctx.download_f32(), e2, "block 2, longer than the raw buffer was")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 11: m17hip_upload_wait at once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pinned", "device"])
def test_upload_wait_at_once_then_the_source_overwritten(cases, chan_s, form):
    """m17hip_upload_wait blocks until the source buffer has been left: it returns no earlier than the channeliser can.  The source (a copy of this case's
    own) is then overwritten — a numpy fill of the pinned block, fill_ on a torch stream and a synchronise for the device block — and run 1's floats and
    records are still block 1's."""
    import torch
    b, D = cases["i16"], chan_s["i16"]
    mine = b.pin.clone().pin_memory() if form == "pinned" else b.dev.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx = context(b.fmt, raw_from=b if form == "pinned" else None)
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
        _waited(t_s, t_c, D, f"m17hip_upload_wait ({form})", t_r)   # (the comparisons first: a source overwritten under the channeliser would show in the words)
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---- 12: m17hip_set_stream at once -----------------------------------------------------------------------------------------------------------------
def test_set_stream_at_once_then_the_run_on_the_new_stream(cases, chan_s):
    """m17hip_set_stream to a torch stream at once behind the staging, then run 1 on that stream: it still waits for the staging."""
    import torch
    b, D = cases["i16"], chan_s["i16"]
    side = torch.cuda.Stream()
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under(t_s, D, "m17hip_set_stream")
        ctx.set_stream(side.cuda_stream)
        assert ctx.stream == side.cuda_stream
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "the floats run 1 read on the new stream")
        _block_2(ctx, b)
        _words(ctx.download_f32(), b.behind_block_1().block(T1, T1 + TB), "block 2, in place on the new stream")
        ctx.upload_wait()
    finally:
        ctx.close()
        torch.cuda.synchronize()


# ---- 13: a narrowband block at once behind the run -------------------------------------------------------------------------------------------------
def test_narrowband_block_at_once_behind_the_run(cases, chan_s):
    """m17hip_upload_iq_device, in place on the main stream, at once behind block 1's run: the discriminator takes each channel's first output against the
    channeliser's last z, which wide_carry_kernel leaves on the copy stream."""
    b, D = cases["i16"], chan_s["i16"]
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
        _made_under(t_s, D, "m17hip_upload_iq_device")
        ctx.upload_iq_device(zdev.data_ptr(), ALL, TB, pitch=TB, iq_format=iq.IQ_I16)
        _words(ctx.download_f32(), e, "a narrowband block behind a channelised block in flight")
        _run_1_is(ctx, b, b.idle)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 14: close() at once ---------------------------------------------------------------------------------------------------------------------------
def test_close_at_once_then_a_fresh_context_on_the_parked_streams(cases, chan_s):
    """m17hip_ctx_destroy at once behind the staging; the next fresh context takes the stream set the closed one parked and channelises one small block to
    the host form's words."""
    b, D = cases["i16"], chan_s["i16"]
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under(t_s, D, "m17hip_ctx_destroy")
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


# ---- 15: table ownership under flight --------------------------------------------------------------------------------------------------------------
def test_the_tuners_table_call_is_refused_under_the_channeliser_and_changes_nothing(cases, chan_s):
    """m17hip_wide_channels at once behind the staging returns M17HIP_ESTATE under the channeliser, without waiting, and changes nothing: block 1 and the
    block behind it have the base table's words."""
    b, D = cases["i16"], chan_s["i16"]
    _, src, bins = table(1)
    s, w = np.ascontiguousarray(rep_src(src), dtype=np.uint32), np.ascontiguousarray(rep(bins), dtype=np.int32)
    e2 = b.behind_block_1().block(T1, T1 + TB)
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        assert ctx.lib.m17hip_wide_channels(ctx.h, ol._p(s), ol._p(w), C.c_uint32(s.size)) == ESTATE
        _returned_under(t_s, D, "m17hip_wide_channels under a raster")
        ctx.run(channels=ALL, samples=T1)
        _check_words(ctx.download_f32(), b.y1_all, "block 1")
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, the table as it was")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_reconfiguration_between_front_and_run_is_refused_under_the_channeliser(cases, chan_s):
    """m17hip_wide_raster between m17hip_demod_front and its run returns M17HIP_ESTATE (tests/test_gpu_raster_input.py has it on an idle device): here the
    front end is queued at once behind the staging, the channeliser in flight.  Nothing changes: run 1 and the block behind it are the base
    configuration's."""
    b, D = cases["i16"], chan_s["i16"]
    e2 = b.behind_block_1().block(T1, T1 + TB)
    ctx = context(b.fmt)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.front(channels=ALL, samples=T1)
        assert ctx.lib.m17hip_wide_raster(ctx.h, C.c_uint32(NS), C.c_uint32(RASTER_DECIM), C.c_uint32(RASTER_BINS), C.c_int(b.fmt), None, C.c_uint32(0)) == ESTATE
        _returned_under(t_s, D, "m17hip_demod_front and a refused m17hip_wide_raster")
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b, b.idle)
        _check_words(ctx.download_f32(), b.y1_all, "block 1")
        _block_2(ctx, b)
        _words(ctx.download_f32(), e2, "block 2, the configuration as it was")
        ctx.upload_wait()
    finally:
        ctx.close()
