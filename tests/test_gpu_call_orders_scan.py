"""GPU tests of the CARRIER SCAN (ABI 622: m17hip_wide_scan, m17hip_wide_scan_fetch, launch_scan) with the resampling tuner still in flight.
tests/test_gpu_wide_scan.py compares tables on a device that is idle by the time the next host call is made; here the regime is
tests/test_gpu_call_orders_spectrum.py's and its parents', whose fixtures and helpers are imported as they stand: 2 int16 sources at 2.048 MSPS with four
transmissions each, 4096 channels (64 distinct ones held 64 times, every one on a carrier, so every channel is open and the squelched tuner has the
unsquelched one's work), block 1 of T1 outputs staged and the call under test made at once, with nothing synchronising in between.  The premise is the
parents': D from the fixture tuner_s, a call that must not wait returns with t_r - t_s < 0.5 D; the intervals are printed; a case whose premise fails FAILS.

What the scan owns that an idle device cannot test: a turn-taking table of pool marks read from either stream; two planes, flag planes and miss planes that
take turns with the squelch's and are read by the block's squelch kernel and tuner in the host table's place; a carry of words ordered by ev_iq; an event
per block, recorded behind the scan kernel and in front of the tuner.

The layout: 2048 points at hop 2048, a band of 9 kHz, a guard of 9 bins, 10 / 6 dB, hang 1.  Channels 0 - 7 are slots; channel 0 is seeded on empty spectrum
(+1.01 MHz), the others where they stand — on carriers, which they hold and cover.  Block 1 therefore assigns channel 0 to the strongest carrier of its
source that no slot covers, and every other channel's floats and records are the parent's."""
import ctypes as C
import time

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import scan_lib as sc
import spectrum_lib as sp
import squelch_floor_lib as sf
import squelch_lib as sq
import test_gpu_call_orders_spectrum as ps
from test_gpu_call_orders_formats import _check_records, _check_words, _u32
from test_gpu_call_orders_resample import (ALL, CN, FCW, GAIN, RATIO, S, SRC, T1, TB, _stage_1, _words, case, context, first_staging_of_the_process,   # noqa: F401
                                           rows, run0_floats, tuner_s)
from test_gpu_call_orders_spectrum import behind, first_spectrum_of_the_process   # noqa: F401
from test_gpu_call_orders_wide2 import _made_under_the_tuner, _returned_under_the_tuner, rep

pytestmark = pytest.mark.gpu

ESTATE = -4
N, HOP, HANG = 2048, 2048, 1
B = m17hip.wide_squelch_half_bins(9000.0, 48000.0 * RATIO, N)
X = m17hip.wide_scan_guard_bins(9000.0, 48000.0 * RATIO, N)
RO, RC = m17hip.wide_squelch_ratio(10.0), m17hip.wide_squelch_ratio(6.0)
POOL = [1] * 8
EMPTY = m17hip.wide_fcw(1010000.0, RATIO)
OPEN = sq.OPEN


def _table(seeded):
    fcw = np.array(rep(FCW), dtype=np.int64)
    if seeded:
        fcw[0] = EMPTY
    return np.array(rep(SRC), dtype=np.uint32), fcw


def expected(b, a, n, seeded, scan=True):
    """The host form of the block of n outputs at output a as the FIRST block of the scan's and the squelch's feed (the floor forgotten, the hold counts
    zero, the seeds taken; the spectrum's frames placed by the feed's sample count): (words, flags, missed, state, band, floor plane, J)."""
    src, fcw = _table(seeded)
    plane, J, first = sp.planes(b.x, N, HOP, [rows(a), rows(a + n)])[0]
    out = sf.Floor(S, B, RO, RC).block(plane, J)
    squelch = sq.Squelch(src, fcw, out[2], out[3], B, HANG)
    pool = np.zeros(ALL, dtype=np.uint8)
    pool[:len(POOL)] = POOL
    words, flags, missed = sc.Scan(pool, X, fcw).block(plane, J, out, squelch) if scan else (fcw.astype(np.int32), None, None)
    squelch.fcw[:] = words
    state, band = squelch.block(plane, J)
    return words, flags, missed, state, band, out, J


def scan_context(seeded, scan=True):
    ctx = context()
    try:
        src, fcw = _table(seeded)
        ctx.wide_channels(src, fcw)
        ctx.wide_spectrum(N, HOP)
        ctx.wide_squelch(B, np.ones(S, dtype=np.float32), np.ones(S, dtype=np.float32), HANG)
        ctx.wide_squelch_floor(RO, RC)
        if scan:
            ctx.wide_scan(POOL, X)
    except Exception:
        ctx.close()
        raise
    return ctx


def _fetch_is(ctx, e, what, back=0):
    words, flags, missed, state, band, floor, J = e
    w, f, m, assigned = ctx.wide_scan_fetch(back)
    assert np.array_equal(w, words) and np.array_equal(f, flags) and np.array_equal(m, missed), (what, w[:8], words[:8], f[:8], flags[:8], m, missed)
    return assigned


def _squelch_is(ctx, e, what):
    words, flags, missed, state, band, floor, J = e
    o, h, bd, frames = ctx.wide_squelch_fetch()
    assert frames == J and np.array_equal(o, (state & OPEN) != 0) and np.array_equal(h, state & ~np.uint32(OPEN)), what
    assert np.array_equal(_u32(bd), _u32(band)), what
    plane, frames = ctx.wide_squelch_floor_fetch()
    assert np.array_equal(_u32(plane), _u32(floor)), what


def _no_scan(ctx, what):
    fcw, flags, missed = np.zeros(ALL, dtype=np.int32), np.zeros(ALL, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
    for back in (0, 1):
        assert ctx.lib.m17hip_wide_scan_fetch(ctx.h, C.c_uint32(back), ol._p(fcw), ol._p(flags), ol._p(missed), C.c_uint64(ALL), None, None, None) == ESTATE, what


def _run_1_but_channel_0(ctx, b, what):
    """Block 1's run: every channel but channel 0 has the parent's floats and records."""
    ctx.run(channels=ALL, samples=T1)
    ctx.T = T1
    _check_words(ctx.download_f32()[1:], b.y1_all[1:], what)
    recs, want = ctx.frames(), b.idle[1]
    _check_records(recs[recs["channel"] != 0], want[want["channel"] != 0])


def test_the_plan(case):
    """What the host form shows on block 1: every channel open; slot 0 assigned, within 900 Hz of a carrier of its source that no other slot stands on; the
    other slots held where they are; the carriers of each source that no slot covers counted as missed."""
    words, flags, missed, state, band, floor, J = expected(case, 0, T1, True)
    assert J == rows(T1) // N and ((state & OPEN) != 0).all()
    assert flags[0] == sc.SLOT | sc.ASSIGNED and (flags[1:8] == sc.SLOT | sc.HELD).all() and not flags[8:].any()
    assert np.array_equal(words[1:], _table(True)[1][1:].astype(np.int32))
    hz = m17hip.wide_scan_hz(words[:1], 48000.0 * RATIO)[0]
    mine = [m17hip.wide_scan_hz([FCW[c]], 48000.0 * RATIO)[0] for c in range(CN) if SRC[c] == SRC[0]]
    assert min(abs(hz - f) for f in mine) < 900.0, (hz, mine)
    assert all(abs(hz - m17hip.wide_scan_hz([FCW[c]], 48000.0 * RATIO)[0]) > 4500.0 for c in range(1, 8) if SRC[c] == SRC[0])


# ---- 1: the fetch at once behind the staged block 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pinned", "device"])
def test_scan_fetch_at_once_behind_the_staged_block_1(case, tuner_s, form):
    """m17hip_wide_scan_fetch at once behind the staging — made under block 1's tuner (the premise, asserted) — returns the host form's table; Context.run()
    resets channel 0 and run 1 has the parent's records elsewhere.  The event the fetch waits for is recorded behind block 1's spectrum, floor and scan
    kernels and IN FRONT of its tuner on the copy stream; WHEN the fetch returns is printed and not asserted: on the one MI355X run that timed it, it came
    back 6.888 ms after the staging call began with D = 7.544 ms (pinned form) — not before the tuner had nearly ended.  Whether the runtime resolves the
    event late or the copies to pageable memory queue behind the tuner's workgroups was not found (NOTES.md)."""
    b, Dt = case, tuner_s
    e = expected(b, 0, T1, True)
    ctx = scan_context(True)
    try:
        t_s = _stage_1(ctx, b, form)
        _made_under_the_tuner(t_s, Dt, f"m17hip_wide_scan_fetch behind the staged block 1 ({form})")
        assigned = _fetch_is(ctx, e, f"block 1's scan ({form})")
        print(f"[scan] m17hip_wide_scan_fetch ({form}): returned {1e3 * (time.perf_counter() - t_s):.3f} ms after the staging call began (D = {1e3 * Dt:.3f} ms)")
        assert assigned == [0]
        _squelch_is(ctx, e, "block 1's decisions")
        _run_1_but_channel_0(ctx, b, f"block 1 ({form})")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 2: m17hip_wide_scan at once under block 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["staged", "in_place"])
def test_wide_scan_at_once_under_block_1(case, behind, tuner_s, how):
    """Block 1 staged with the scan off; m17hip_wide_scan at once: it waits for nothing, and block 1 keeps the host's table.  Block 2 is the first block of
    the scan's feed: its table, decisions and floats are the host form's, its floor forgotten and taken anew."""
    b, Dt = case, tuner_s
    e2 = expected(b, T1, TB, False)
    assert not (e2[1] & sc.ASSIGNED).any() and (e2[1][:8] == sc.SLOT | sc.HELD).all()   # (every slot on its carrier: the words are the parent's)
    ctx = scan_context(False, scan=False)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_scan(POOL, X)
        _returned_under_the_tuner(t_s, Dt, "m17hip_wide_scan under block 1")
        _no_scan(ctx, "no scanned block yet")
        if how == "in_place":
            ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
            _fetch_is(ctx, e2, "block 2 in place")
            _squelch_is(ctx, e2, "block 2 in place")
            _words(ctx.download_f32(), behind["e2"], "block 2 in place")
            ctx.run(channels=ALL, samples=T1)
        else:
            ctx.run(channels=ALL, samples=T1)
            ctx.upload_wide_device_async(b.at("device", T1), ALL, TB, b.pitch, GAIN)
            _fetch_is(ctx, e2, "block 2 staged")
            _squelch_is(ctx, e2, "block 2 staged")
            ctx.run(channels=ALL, samples=TB)
            ctx.T = TB
            _words(ctx.download_f32(), behind["e2"], "block 2 staged")
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: off at once under a scanned block 1 ------------------------------------------------------------------------------------------------------------------------
def test_scan_off_at_once_under_block_1(case, tuner_s):
    """m17hip_wide_scan(NULL, 0) at once under the scanned block 1: it waits for nothing; block 1, already queued, keeps the scan's table (channel 0 tuned);
    the fetch is M17HIP_ESTATE at once; block 2 sees the host's table again — channel 0 back on its seed, closed — from a fresh feed of decisions."""
    b, Dt = case, tuner_s
    e2 = expected(b, T1, TB, True, scan=False)
    assert not e2[3][0] & OPEN and ((e2[3][1:] & OPEN) != 0).all()
    ctx = scan_context(True)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_scan(None)
        _returned_under_the_tuner(t_s, Dt, "m17hip_wide_scan(NULL, 0) under block 1")
        _no_scan(ctx, "the scan is off")
        _run_1_but_channel_0(ctx, b, "block 1, the scan turned off behind it")
        ctx.T = T1
        assert (ctx.download_f32()[0] != 0).any()   # (channel 0 was tuned by block 1's scan, not left closed on its seed)
        ctx.upload_wide_device(b.at("device", T1), ALL, TB, b.pitch, GAIN)
        _squelch_is(ctx, e2, "block 2 under the host's table")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4: a reconfiguration of the spectrum at once under a scanned block 1 --------------------------------------------------------------------------------------------
def test_wide_spectrum_at_once_under_a_scanned_block_1(case, tuner_s):
    """m17hip_wide_spectrum at once under the scanned block 1 turns the squelch and the scan off and waits for nothing; block 1 keeps its table; turning the
    scan on again needs the squelch and the floor first."""
    b, Dt = case, tuner_s
    ctx = scan_context(True)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_spectrum(64, 64)
        _returned_under_the_tuner(t_s, Dt, "m17hip_wide_spectrum under the scanned block 1")
        _no_scan(ctx, "the scan went with the squelch")
        pool = np.ones(8, dtype=np.uint8)
        assert ctx.lib.m17hip_wide_scan(ctx.h, ol._p(pool), C.c_uint32(8), C.c_uint32(X)) == ESTATE
        _run_1_but_channel_0(ctx, b, "block 1, the spectrum changed behind it")
        ctx.upload_wait()
    finally:
        ctx.close()
