"""GPU tests of the SOURCE SPECTRUM (ABI 616: m17hip_wide_spectrum, m17hip_wide_spectrum_fetch, launch_spectrum) with the resampling tuner still in flight.
tests/test_gpu_spectrum.py compares planes on a device that is idle by the time the next host call is made (blocks of a few hundred samples); here the
regime is tests/test_gpu_call_orders_resample.py's, whose fixtures and helpers — and its parents' — are imported as they stand: 2 int16 sources at
2.048 MSPS, 4096 channels (64 distinct ones held 64 times), block 1 of T1 outputs (204 800 samples a source) staged and the call under test made at once,
with nothing synchronising in between; the blocks behind it have TB outputs (16 384 samples) or T1 + 192 (212 992).  context() is the parent's with
m17hip_wide_spectrum called after its reset.  The premise is the parent's as well: D from its fixture tuner_s (the spectrum adds microseconds to a tuner of
milliseconds), a call that must not wait returns with t_r - t_s < 0.5 D, one that must wait was made with t_c - t_s < 0.5 D and returned with
t_r - t_s >= 0.5 D; the intervals are printed; a case whose premise fails FAILS.

What the spectrum owns that an idle device cannot test: one scratch buffer and two planes that take turns, shared by blocks tuned on the copy stream
(staged) and on the main stream (in place) and ordered by ev_iq alone; the scratch regrown behind a host wait for ev_iq; the planes regrown where `points`
has risen; a turn-taking device table for window and twiddles read from either stream; an event per plane and a fetch stream of its own.

Expected planes are spectrum_lib.planes on the parent's case.x, compared as uint32 words with J and first_sample (test_gpu_spectrum._expect_plane).  In
every case the channels' floats are the parent's words and run 1's records and m17_diag the parent's, byte for byte: the spectrum moves none of them.
"""
import time

import numpy as np
import pytest

import m17hip
import spectrum_lib as sp
import test_gpu_call_orders_resample as pr
import test_gpu_call_orders_wide2 as p2
import test_gpu_spectrum as gs
from test_gpu_call_orders_formats import _check_words, _in_flight, _u32
from test_gpu_call_orders_resample import (ALL, CN, FCW, FMT, GAIN, LISTED, OTHER2, OTHER_R, S, SRC, T0F, T1, TB, U, _kept_carries, _run_1_is,   # noqa: F401
                                           _stage_1, _words, case, context, feeds, first_staging_of_the_process, rows, run0_floats, taps, tuner_s)
from test_gpu_call_orders_wide2 import _made_under_the_tuner, _returned_under_the_tuner, _waited

pytestmark = pytest.mark.gpu

ESTATE = gs.ESTATE
N2 = T1 + 192                # outputs of the block that outgrows the scratch
DEFAULT = (1024, 1024)       # points and hop where a case is about something else
_PLANES = {}


def ramp(N):
    return (0.25 + np.arange(N) / N).astype(np.float32)


def plane(b, N, hop, a, n, win=None, fresh=False):
    """(plane [S][N], J, first_sample) of the block of n outputs that begins at output a of the parent's sources: the host form's, computed once.  fresh:
    the feed starts over at that block (count 0)."""
    key = (N, hop, a, n, None if win is None else win.tobytes(), fresh)
    if key not in _PLANES:
        lo, hi = rows(a), rows(a + n)
        if fresh:
            _PLANES[key] = sp.planes(b.x[:, lo:hi], N, hop, [0, hi - lo], win)[0]
        else:
            _PLANES[key] = sp.planes(b.x, N, hop, [lo, hi], win)[0]
        assert _PLANES[key][1] == sp.frames_stated(0 if fresh else lo, hi - lo, N, hop)[1]
    return _PLANES[key]


def spectrum_context(N, hop, win=None, maxT=T1):
    ctx = context(maxT)
    try:
        ctx.wide_spectrum(N, hop, win)
    except Exception:
        ctx.close()
        raise
    return ctx


def _plane_is(ctx, N, exp, what, back=0):
    gs._expect_plane(ctx, S, N, exp, what, back)


def _no_plane(ctx, N, what, backs=(0, 1)):
    for back in backs:
        assert gs._fetch(ctx, S, N, back)[0] == ESTATE, (what, back)


def _stage(ctx, b, a, n):
    ctx.upload_wide_device_async(b.at("device", a), ALL, n, b.pitch, GAIN)


def _in_place(ctx, b, a, n):
    ctx.upload_wide_device(b.at("device", a), ALL, n, b.pitch, GAIN)


def _floats_are(ctx, n, exp64, what):
    """The float slab's rows of n samples against the 64 distinct channels' words."""
    ctx.T = n
    _words(ctx.download_f32(), exp64, what)


def _floats_of_block_1(ctx, b, what):
    ctx.T = T1
    _check_words(ctx.download_f32(), b.y1_all, what)


@pytest.fixture(scope="module", autouse=True)
def first_spectrum_of_the_process(first_staging_of_the_process):
    """One spectrum block at every size the cases use, staged and in place, on a throwaway context: the kernels' first launches of the process and the fetch
    stream's creation lie outside every interval a case measures."""
    import torch
    quiet = torch.zeros((S, rows(TB), 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx = context(TB)
    try:
        for N in (64, 1024, 4096):
            ctx.wide_spectrum(N, N)
            ctx.upload_wide_device(quiet.data_ptr(), ALL, TB, rows(TB))
            ctx.run()
            ctx.upload_wide_device_async(quiet.data_ptr(), ALL, TB, rows(TB))
            ctx.run(channels=ALL, samples=TB)
            ctx.frames()
            assert ctx.wide_spectrum_fetch()[1] == rows(TB) // N
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def behind(case):
    """The host form's floats of the blocks behind block 1, each computed once: block 2 of TB outputs, block 3 of TB outputs behind it, and the block of
    T1 + 192 outputs."""
    r = case.behind_block_1()
    e2 = r.block(T1, T1 + TB)
    e3 = r.block(T1 + TB, T1 + 2 * TB)
    long2 = case.behind_block_1().block(T1, T1 + N2)
    first = feeds(case.x).block(0, TB)
    for a in (e2, e3, long2, first):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return {"e2": e2, "e3": e3, "long2": long2, "first": first}


# ---- 1: a fetch at once behind the staged block 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 64])
@pytest.mark.parametrize("form", ["pinned", "device"])
def test_fetch_at_once_behind_the_staged_block_1(case, tuner_s, form, N):
    """m17hip_wide_spectrum_fetch(back = 0) at once behind the staging waits for block 1's spectrum kernels, which follow its tuner on the copy stream, and
    returns the host form's plane (50 frames of 4096 points; 3200 frames of 64); back = 1 is M17HIP_ESTATE.  Run 1 then has the parent's records."""
    b, Dt = case, tuner_s
    exp = plane(b, N, N, 0, T1)
    assert exp[1] == rows(T1) // N and exp[2] == 0
    ctx = spectrum_context(N, N)
    try:
        t_s = _stage_1(ctx, b, form)
        t_c = time.perf_counter()
        code, got, j, f = gs._fetch(ctx, S, N, 0)
        t_r = time.perf_counter()
        assert code == 0 and (j, f) == (exp[1], exp[2]), (code, j, f)
        gs._assert_words(got, exp[0], f"block 1's plane ({form}, {N})")
        _no_plane(ctx, N, "one block only", backs=(1,))
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b.idle)
        _floats_of_block_1(ctx, b, "the floats run 1 read")
        ctx.upload_wait()
        _waited(t_s, t_c, Dt, f"m17hip_wide_spectrum_fetch ({form}, {N} points)", t_r)
    finally:
        ctx.close()


# ---- 2: a fetch does not wait for a run -----------------------------------------------------------------------------------------------------------------
def test_fetch_does_not_wait_for_a_run_in_flight(case, behind, run0_floats):
    """The parent's float run 0 is in flight on the main stream (asserted), a block of TB outputs is staged and its plane fetched at once: the plane is the
    host form's, and the main stream STILL has work outstanding after the fetch has returned — the fetch waited for the block's event, not for the run."""
    b = case
    N, hop = DEFAULT
    exp = plane(b, N, hop, 0, TB)
    assert exp[1] == rows(TB) // N
    ctx = spectrum_context(N, hop, maxT=T0F)
    try:
        import torch
        ctx.upload_device(run0_floats[1].data_ptr(), ALL, T0F, dtype=np.float32)
        t_0 = time.perf_counter()
        ctx.run()
        _in_flight(ctx)
        t_s = time.perf_counter()
        _stage(ctx, b, 0, TB)
        code, got, j, f = gs._fetch(ctx, S, N, 0)
        t_r = time.perf_counter()
        _in_flight(ctx, "run 0 (after the fetch has returned)")
        torch.cuda.ExternalStream(ctx.stream).synchronize()
        print(f"[spectrum] a fetch beside run 0: returned {1e3 * (t_r - t_s):.3f} ms after the staging call began ({1e3 * (t_r - t_0):.3f} ms after run 0 was "
              f"queued), run 0 still in flight; its main stream was idle {1e3 * (time.perf_counter() - t_0):.3f} ms after it was queued")
        assert code == 0 and (j, f) == (exp[1], exp[2])
        gs._assert_words(got, exp[0], "the staged block's plane beside a run in flight")
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), behind["first"], "the floats of the staged block")
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: m17hip_wide_spectrum at once under block 1 -------------------------------------------------------------------------------------------------------
def _block_2_behind_block_1(ctx, b, Dt, t_s, how, e2, what, n=TB):
    """Block 2 of n outputs made at once, in place on the main stream before block 1's run (the parent's case 2) or staged behind block 1's run; block 1's
    and block 2's floats and run 1's records are the parent's.  On return the latest block is block 2."""
    if how == "in_place":
        _made_under_the_tuner(t_s, Dt, f"m17hip_upload_wide_device in front of block 1's run ({what})")
        _in_place(ctx, b, T1, n)
        print(f"[spectrum] block 2 in place ({what}): returned {1e3 * (time.perf_counter() - t_s):.3f} ms after block 1's staging call began")
        _words(ctx.download_f32(), e2, f"block 2 in place ({what})")
        ctx.run(channels=ALL, samples=T1)
        _floats_of_block_1(ctx, b, f"block 1, run behind block 2 ({what})")
        _run_1_is(ctx, b.idle)
    else:
        ctx.run(channels=ALL, samples=T1)
        _made_under_the_tuner(t_s, Dt, f"m17hip_upload_wide_device_async behind block 1's run ({what})")
        _stage(ctx, b, T1, n)
        print(f"[spectrum] block 2 staged ({what}): returned {1e3 * (time.perf_counter() - t_s):.3f} ms after block 1's staging call began")
        _floats_of_block_1(ctx, b, f"block 1 ({what})")
        _run_1_is(ctx, b.idle)
        ctx.run(channels=ALL, samples=n)
        _floats_are(ctx, n, e2, f"block 2 staged ({what})")
        ctx.frames()


CHANGES = {"points_64_to_4096": ((64, 64, None), (4096, 4096, None)), "points_4096_to_64": ((4096, 4096, None), (64, 64, None)),
           "a_callers_window": ((1024, 1024, None), (1024, 1024, ramp(1024)))}


@pytest.mark.parametrize("how", ["staged", "in_place"])
@pytest.mark.parametrize("change", list(CHANGES))
def test_wide_spectrum_at_once_under_block_1(case, behind, tuner_s, change, how):
    """m17hip_wide_spectrum returns under the tuner.  Block 1's plane is forgotten — both values of `back` are M17HIP_ESTATE until block 2 —; block 2, made
    at once, has the host form's plane under the NEW table at the feed's count 204 800.  Where `points` rises the planes are regrown while block 1's
    kernels may still write the old ones; where it falls or stays the table alone takes its turn."""
    b, Dt = case, tuner_s
    (Na, ha, wa), (Nb, hb, wb) = CHANGES[change]
    exp = plane(b, Nb, hb, T1, TB, wb)
    assert exp[1] > 0 and exp[2] == rows(T1) + (-rows(T1)) % hb
    if Na == Nb:
        assert (_u32(exp[0]) != _u32(plane(b, Na, ha, T1, TB, wa)[0])).any(), "the window decides block 2's plane"
    ctx = spectrum_context(Na, ha, wa)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_spectrum(Nb, hb, wb)
        _returned_under_the_tuner(t_s, Dt, f"m17hip_wide_spectrum ({change})")
        _no_plane(ctx, Nb, "block 1's plane is forgotten")
        _block_2_behind_block_1(ctx, b, Dt, t_s, how, behind["e2"], change)
        _plane_is(ctx, Nb, exp, f"block 2 under the new table ({change}, {how})")
        _no_plane(ctx, Nb, "block 1's plane stays forgotten", backs=(1,))
        ctx.upload_wait()
    finally:
        ctx.close()


@pytest.mark.parametrize("fetch_between", [False, True], ids=["no_fetch_between", "block_2_fetched"])
def test_two_changes_in_a_row_across_three_staged_blocks(case, behind, tuner_s, fetch_between):
    """Blocks 1, 2 and 3 staged back to back, each with its run, and a new window in front of blocks 2 and 3: both copies of the device table are written
    while launches that read the copy before are queued, and the third write has to wait for block 1's reader.  A change forgets the planes, so block 2's
    plane can only be fetched in front of the second change: with no fetch in between block 3's plane is compared with the third window's; with block 2
    fetched, each of the two with the window it was uploaded under."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    w2, w3 = ramp(N), ramp(N)[::-1].copy()
    exp2, exp3 = plane(b, N, hop, T1, TB, w2), plane(b, N, hop, T1 + TB, TB, w3)
    assert (_u32(exp3[0]) != _u32(plane(b, N, hop, T1 + TB, TB, w2)[0])).any() and (_u32(exp3[0]) != _u32(plane(b, N, hop, T1 + TB, TB)[0])).any()
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_spectrum(N, hop, w2)
        ctx.run(channels=ALL, samples=T1)
        _stage(ctx, b, T1, TB)
        _returned_under_the_tuner(t_s, Dt, "block 2's staging behind the first change")
        if fetch_between:
            _plane_is(ctx, N, exp2, "block 2 under the second window")
        ctx.wide_spectrum(N, hop, w3)
        ctx.run(channels=ALL, samples=TB)
        if not fetch_between:
            _made_under_the_tuner(t_s, Dt, "block 3's staging behind the second change")
        _stage(ctx, b, T1 + TB, TB)
        _plane_is(ctx, N, exp3, "block 3 under the third window")
        _no_plane(ctx, N, "block 2's plane is forgotten", backs=(1,))
        ctx.run(channels=ALL, samples=TB)
        _words(ctx.download_f32(), behind["e3"], "block 3's floats")
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 4: off at once under block 1 ----------------------------------------------------------------------------------------------------------------------------
def test_off_at_once_under_block_1(case, behind, tuner_s):
    """m17hip_wide_spectrum(0) returns under the tuner; block 2 queues no spectrum (the timer's launch count, with timing turned on behind the measured
    interval, stays where it was while the tuner's goes up by one) and the fetch is M17HIP_ESTATE."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.wide_spectrum(0, 0)
        _returned_under_the_tuner(t_s, Dt, "m17hip_wide_spectrum(0)")
        ctx.run(channels=ALL, samples=T1)
        ctx.timing(True)
        ctx.timing_reset()
        n_sp, n_tune = ctx.timing_get("spectrum")[1], ctx.timing_get("resample")[1]
        _stage(ctx, b, T1, TB)
        _floats_of_block_1(ctx, b, "block 1")
        _run_1_is(ctx, b.idle)
        ctx.run(channels=ALL, samples=TB)
        _floats_are(ctx, TB, behind["e2"], "block 2, no spectrum beside it")
        ctx.frames()
        assert ctx.timing_get("spectrum")[1] == n_sp and ctx.timing_get("resample")[1] == n_tune + 1
        ctx.timing(False)
        _no_plane(ctx, N, "the spectrum is off")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: the scratch outgrown by block 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["in_place", "staged"])
def test_scratch_outgrown_by_block_2_while_block_1_is_in_flight(case, behind, tuner_s, how):
    """N = 1024, hop = 12 800: block 1 has 16 frames (one group of 16), the block of T1 + 192 outputs behind it, which begins at count 204 800 = 16 x 12 800,
    has 17 (two groups): the scratch is regrown, behind a host wait for ev_iq, while block 1's kernels may still write it.  Both planes are the host
    form's afterwards, and both blocks' floats the parent's."""
    b, Dt = case, tuner_s
    N, hop = 1024, 12800
    assert sp.frames_stated(0, rows(T1), N, hop) == (0, 16) and sp.frames(0, rows(T1), N, hop) == (0, 16)
    assert rows(T1) == 16 * hop and sp.frames_stated(rows(T1), rows(N2), N, hop) == (0, 17) and sp.frames(rows(T1), rows(N2), N, hop) == (0, 17)
    exp1, exp2 = plane(b, N, hop, 0, T1), plane(b, N, hop, T1, N2)
    assert (exp1[1], exp1[2], exp2[1], exp2[2]) == (16, 0, 17, rows(T1))
    ctx = spectrum_context(N, hop, maxT=N2)
    try:
        t_s = _stage_1(ctx, b, "device")
        _block_2_behind_block_1(ctx, b, Dt, t_s, how, behind["long2"], "two groups behind one", n=N2)
        _plane_is(ctx, N, exp2, f"block 2, two groups ({how})", back=0)
        _plane_is(ctx, N, exp1, f"block 1, one group ({how})", back=1)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 6: three blocks, alternating streams -----------------------------------------------------------------------------------------------------------------------
def test_three_blocks_on_alternating_streams_and_no_fetch_in_between(case, behind, tuner_s):
    """Block 1 staged (copy stream), block 2 in place at once (main stream: the parent's test_block_2_in_place_at_once_before_block_1s_run with the spectrum
    on), block 1's run, block 3 staged at once (copy stream) — and only then the fetches: back = 0 is block 3's plane, back = 1 block 2's.  Block 3 wrote
    the plane block 1 had and all three used one scratch: nothing but ev_iq ordered them."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    exp2, exp3 = plane(b, N, hop, T1, TB), plane(b, N, hop, T1 + TB, TB)
    assert (_u32(exp3[0]) != _u32(plane(b, N, hop, 0, T1)[0])).any() and exp3[2] == rows(T1 + TB)
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, Dt, "block 2 in place in front of block 1's run")
        _in_place(ctx, b, T1, TB)
        ctx.run(channels=ALL, samples=T1)
        _stage(ctx, b, T1 + TB, TB)
        _plane_is(ctx, N, exp3, "block 3, staged", back=0)
        _plane_is(ctx, N, exp2, "block 2, in place", back=1)
        _floats_of_block_1(ctx, b, "block 1, run behind block 2's upload")
        _run_1_is(ctx, b.idle)
        ctx.run(channels=ALL, samples=TB)
        _floats_are(ctx, TB, behind["e3"], "block 3 continues blocks 1 and 2")
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 7: the resets ---------------------------------------------------------------------------------------------------------------------------------------------
def test_full_reset_at_once_under_block_1(case, tuner_s):
    """m17hip_demod_reset at once under block 1: the planes are forgotten, and the next block is the first of a fresh feed — its first_sample counts from 0,
    its plane and its floats are the host form's for that block alone."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    exp = plane(b, N, hop, T1, TB, fresh=True)
    assert exp[2] == 0 and exp[1] == rows(TB) // N
    e = feeds(b.x[:, rows(T1):]).block(0, TB)
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        _made_under_the_tuner(t_s, Dt, "m17hip_demod_reset")
        ctx.reset()
        _no_plane(ctx, N, "a reset forgets the planes")
        _in_place(ctx, b, T1, TB)
        _plane_is(ctx, N, exp, "the first block of the feed behind the reset")
        _no_plane(ctx, N, "one block only", backs=(1,))
        _words(ctx.download_f32(), e, "the first block of the feed behind the reset")
        ctx.upload_wait()
    finally:
        ctx.close()


def test_channel_reset_at_once_under_block_1(case, behind, tuner_s):
    """m17hip_demod_reset_channels (the parent's list) at once under block 1 leaves feed, count and planes alone: the fetch still returns block 1's plane,
    block 2's begins at count 204 800, and the floats are the parent's (the listed channels' first output +0)."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    exp1, exp2 = plane(b, N, hop, 0, T1), plane(b, N, hop, T1, TB)
    ref = b.behind_block_1()
    for c in LISTED:
        ref.carry[c] = np.zeros(2, dtype=np.float32)
    every = p2.rep(behind["e2"])
    every[:CN] = ref.block(T1, T1 + TB)
    assert (every[LISTED, 0] == 0).all() and (behind["e2"][LISTED, 0] != 0).all()
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        ctx.reset_channels(LISTED)
        _returned_under_the_tuner(t_s, Dt, "m17hip_demod_reset_channels")
        _plane_is(ctx, N, exp1, "block 1's plane behind the reset of single channels")
        ctx.run(channels=ALL, samples=T1)
        _floats_of_block_1(ctx, b, "block 1, staged before the reset")
        _stage(ctx, b, T1, TB)
        ctx.run(channels=ALL, samples=TB)
        ctx.T = TB
        _check_words(ctx.download_f32(), every, "block 2 behind the reset")
        _plane_is(ctx, N, exp2, "block 2's plane")
        _plane_is(ctx, N, exp1, "block 1's plane, now the block before", back=1)
        ctx.frames()
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 8: a configuration call at once under a spectrum block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("to", ["resample", "config2"])
def test_reconfiguration_at_once_under_a_spectrum_block(case, tuner_s, to):
    """m17hip_wide_resample to another ratio and m17hip_wide_config2 at once under block 1 and its spectrum: the call frees the scratch and both planes, so
    it waits (wide_setup's host wait for ev_iq).  The spectrum is off behind it — M17HIP_ESTATE, and no launch on its timer —, run 1 is the old
    configuration's, and a block under the new one has that configuration's host-form floats with the carries kept (the parent's case 5)."""
    b, Dt = case, tuner_s
    N, hop = DEFAULT
    rest = b.x[:, rows(T1):]
    if to == "resample":
        e2 = _kept_carries(feeds(rest, shape=OTHER_R), b.ref1.carry, OTHER_R[1])
    else:
        t1, t2 = m17hip.wide_default_taps2(*OTHER2)
        e2 = _kept_carries(p2.PFeeds2(rest, t1, OTHER2[0], t2, OTHER2[1], SRC, FCW, GAIN), b.ref1.carry, 4)
    ctx = spectrum_context(N, hop)
    try:
        t_s = _stage_1(ctx, b, "device")
        t_c = time.perf_counter()
        if to == "resample":
            ctx.wide_resample(S, *OTHER_R, FMT)
        else:
            ctx.wide_config2(S, OTHER2[0], OTHER2[1], FMT)
        _waited(t_s, t_c, Dt, f"m17hip_wide_{to} under a spectrum block")
        _no_plane(ctx, N, "a configuration call turns the spectrum off")
        ctx.run(channels=ALL, samples=T1)
        _run_1_is(ctx, b.idle)
        _floats_of_block_1(ctx, b, "block 1, tuned with the configuration before")
        ctx.timing(True)
        ctx.timing_reset()
        _in_place(ctx, b, T1, TB)
        _words(ctx.download_f32(), e2, "block 2, a fresh feed of the new configuration")
        assert ctx.timing_get("spectrum")[1] == 0 and ctx.timing_get("resample" if to == "resample" else "tune2")[1] == 1
        ctx.timing(False)
        _no_plane(ctx, N, "the spectrum stays off")
        ctx.upload_wait()
    finally:
        ctx.close()
