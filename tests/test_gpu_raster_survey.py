"""GPU tests of the raster survey (ABI 613, include/m17hip.h: m17hip_wide_survey): chan_survey_kernel computes the channeliser's z for ALL bins of every
source at the block's survey times and sums their power per group of 16 times, chan_survey_sum_kernel adds the groups.  Every comparison is exact: the
plane (m17hip_wide_survey_fetch) as uint32 words against the HOST form of the same arithmetic (tests/survey_lib.py: raster_lib's z, detail/core.h's
chan_power and two-level sum under the host compiler) — NaN-ness where that is a NaN.  What the host form itself is worth is asserted without a GPU in
tests/test_raster_survey.py.  The helpers of tests/test_gpu_raster_input.py are imported as they stand."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import raster_lib as rl
import survey_lib as sl
import test_gpu_raster_input as gr
import test_gpu_wide_input as g1
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS, SB = g1.FMTS, g1.SB
_raster, _channels, _data, _dev, _raw = gr._raster, gr._channels, gr._data, gr._dev, gr._raw
_u32, _assert_words = g1._u32, g1._assert_words


def _survey(ctx, stride):
    return ctx.lib.m17hip_wide_survey(ctx.h, C.c_uint32(stride))


def _fetch(ctx, S, M, back=0, capacity=None, null=False):
    """(code, plane [S][M], times, first_output); the buffer is pre-filled with 7 so that a refusal that writes shows."""
    buf = np.full(S * M, 7.0, dtype=np.float32)
    t, n0 = C.c_uint32(0xFFFFFFFF), C.c_uint64(0xFFFFFFFFFFFFFFFF)
    code = ctx.lib.m17hip_wide_survey_fetch(ctx.h, C.c_uint32(back), None if null else ol._p(buf), C.c_uint64(buf.size if capacity is None else capacity),
                                            C.byref(t), C.byref(n0))
    return code, buf.reshape(S, M), t.value, n0.value


def _expect_plane(ctx, S, M, exp, what, back=0):
    plane, J, N0 = exp
    code, got, t, n0 = _fetch(ctx, S, M, back)
    assert code == 0, (what, code)
    assert (t, n0) == (J, N0), (what, t, n0, J, N0)
    _assert_words(got, plane, what)


def _hop(M, R, L, fmt, cases, S, seed, taps=None, bad=None):
    """Fresh feeds of S sources, ONE channel (source 0, bin 0): no channel listens to the other sources, which chan_kernel therefore skips.  cases:
    (stride, outputs) pairs, each from a reset feed, in place from device memory."""
    rng = np.random.default_rng(seed)
    Tmax = max(T for _, T in cases)
    P = Tmax * R + 3   # odd: rows are not 16-byte aligned
    host = _data(fmt, S, P, rng, bad)
    dev = _dev(host)
    if taps is None:
        taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    ctx = m17hip.Context(1, Tmax)
    try:
        assert _raster(ctx, S, R, M, fmt, taps) == 0
        assert _channels(ctx, [0], [0]) == 0
        for stride, T in cases:
            exp = sl.planes([host[s][: T * R] for s in range(S)], taps, R, M, stride, [0, T])[0]
            assert exp[1] == T // stride and exp[2] == 0
            if bad is not None and fmt == wl.IQ_F32:
                assert np.isfinite(exp[0][[s for s in range(S) if s != bad]]).all() and not np.isfinite(exp[0][bad]).all()
            elif exp[1]:
                assert np.isfinite(exp[0]).all() and (exp[0] > 0).any()
            ctx.reset()
            assert _survey(ctx, stride) == 0
            assert _raw(ctx, "m17hip_upload_wide_device", dev.data_ptr(), 1, T, P) == 0
            _expect_plane(ctx, S, M, exp, (M, R, L, fmt, stride, T))
    finally:
        ctx.close()


# ---- 1: one hop ----------------------------------------------------------------------------------------------------------------------------------
STRIDES = (1, 3, 16, 17)
JS = (0, 1, 15, 16, 17, 33)


@pytest.mark.parametrize("shape", rl.SMALL, ids=["M{}_R{}_L{}".format(*s) for s in rl.SMALL])
def test_survey_small_shapes(shape):
    """The shapes where indexing can go wrong x strides 1, 3, 16, 17 x block lengths that give J = 0, 1, 15, 16, 17, 33 survey times (a group's edges, two
    groups and three; an odd output more where the stride leaves room).  Two sources, and source 1 has NO channel listening: its plane is right all the
    same."""
    M, R, L = shape
    cases = []
    for stride in STRIDES:
        for J in JS:
            T = J * stride + (1 if stride > 1 else 0)
            if T:
                cases.append((stride, T))
    assert {T // s for s, T in cases} == set(JS)
    _hop(M, R, L, wl.IQ_I16, cases, 2, 6300 + M + R + L)


@pytest.mark.parametrize("fmt", list(FMTS), ids=list(FMTS))
def test_survey_192_bins_of_a_2400k_source(fmt):
    """M = 192, decim 50, the 1601 default taps, 300 outputs at stride 7 (42 times: two groups of 16 and one of 10; the windows overlap and three times
    make a sub-tile), two sources of which only source 0 is listened to.  In float32 source 1 holds infinities and NaNs: its row is non-finite where the host form says so, and
    source 0's row is finite and exact."""
    M, R = 192, 50
    taps = m17hip.wide_raster_default_taps(R)
    assert taps.size == 1601 and sl.tile_and_lds(1601, R, M, 7)[0] == 3 and sl.tile_and_lds(1601, R, M, 48) == (1, 17432)
    _hop(M, R, 1601, FMTS[fmt], [(7, 300)], 2, 6310 + FMTS[fmt], taps=taps, bad=1)


def test_survey_at_the_limits_of_its_configuration():
    """M = 256, decim 64, 4096 taps: one survey time per sub-tile (its window alone is 32 KB of LDS), 40 outputs at stride 1 — and it must launch."""
    assert sl.tile_and_lds(4096, 64, 256, 64) == (1, 38928) and sl.tile_and_lds(4096, 64, 256, 1)[1] <= 65536
    _hop(256, 64, 4096, wl.IQ_I16, [(1, 40)], 2, 6320)


def test_survey_windows_that_overlap_touch_and_stand_apart():
    """stride * decim below, at and above the taps' length: one run of samples serves all times of a sub-tile, or each has a window of its own."""
    M, R, L = 12, 4, 40
    _hop(M, R, L, wl.IQ_U8, [(2, 70), (9, 200), (10, 200), (11, 200), (40, 700)], 2, 6325)


def test_survey_sub_tiles_of_three_and_of_five_times():
    """M = 64, decim 5, 1000 taps: at stride 200 the windows stand apart and three fit a sub-tile, at stride 100 they overlap and five do.  17 and 33 times:
    groups of 16 go through sub-tiles of 3, 3, 3, 3, 3, 1 and of 5, 5, 5, 1, and a group of one time follows."""
    M, R, L = 64, 5, 1000
    assert sl.tile_and_lds(L, R, M, 200)[0] == 3 and sl.tile_and_lds(L, R, M, 100)[0] == 5
    _hop(M, R, L, wl.IQ_I16, [(200, 17 * 200 + 7), (100, 33 * 100), (100, 1700)], 2, 6327)


# ---- 2: the feed ---------------------------------------------------------------------------------------------------------------------------------
FEED_M, FEED_R, FEED_L, FEED_S, FEED_C = gr.FEED_M, gr.FEED_R, gr.FEED_L, gr.FEED_S, gr.FEED_C
FEED_LENS = (1, 2, 255, 1, 300, 3, 200)
FEED_CUTS = np.cumsum((0,) + FEED_LENS).tolist()
FEED_STRIDE = 7


def test_a_feed_in_ragged_blocks_is_surveyed_block_by_block():
    """Blocks of 1, 2, 255, 1, 300, 3 and 200 outputs at stride 7 — through the host form, in place from device memory and staged from device memory by
    turns: per block the plane, J (0 for the first two blocks) and N0 are the host form's, whichever stream the
    block ran on; the scratch grows with the first block that has more groups."""
    x, taps = gr._feed_case(seed=6330)
    R, M = FEED_R, FEED_M
    exp = sl.planes(x, taps, R, M, FEED_STRIDE, FEED_CUTS)
    assert [e[1] for e in exp] == [b // FEED_STRIDE - a // FEED_STRIDE for a, b in zip(FEED_CUTS[:-1], FEED_CUTS[1:])] and 0 in [e[1] for e in exp]
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(FEED_C, max(FEED_LENS))
    try:
        ctx.wide_raster(FEED_S, R, M, wl.IQ_I16, taps)
        ctx.wide_raster_channels(gr.FEED_SRC, gr.FEED_BINS)
        ctx.reset()
        ctx.wide_survey(FEED_STRIDE)
        how = ["in_place", "staged_device", "host", "staged_device", "staged_device", "in_place", "host"]
        for k, ((a, b), h) in enumerate(zip(zip(FEED_CUTS[:-1], FEED_CUTS[1:]), how)):
            off = a * R * sb
            if h == "in_place":
                ctx.upload_wide_device(dev.data_ptr() + off, FEED_C, b - a, W, gr.FEED_GAIN)
            elif h == "host":
                ctx.upload_wide(x[:, a * R: b * R], gain=gr.FEED_GAIN)
            else:
                ctx.upload_wide_device_async(dev.data_ptr() + off, FEED_C, b - a, W, gr.FEED_GAIN)
                ctx.run(channels=FEED_C, samples=b - a)
            _expect_plane(ctx, FEED_S, M, exp[k], (h, a, b))
            if k:
                _expect_plane(ctx, FEED_S, M, exp[k - 1], (h, a, b, "the block before"), back=1)
        ctx.upload_wait()
        power, times, first = ctx.wide_survey_fetch()
        assert power.shape == (FEED_S, M) and power.dtype == np.float32 and (times, first) == exp[-1][1:]
        _assert_words(power, exp[-1][0], "Context.wide_survey_fetch")
    finally:
        ctx.close()


def test_a_fetch_behind_a_queued_run_and_a_later_staged_block_names_the_right_planes():
    """Block A staged, its run queued, block B staged — and only then the fetches: back = 1 is A's plane, back = 0 is B's.  (No timing is asserted: what
    the fetch waits for is the plane's own event.)  B's run and a third block in place follow, and the planes move on by one."""
    T = 192 * 5
    x, taps = gr._feed_case(seed=6340, outputs=3 * T)
    R, M = FEED_R, FEED_M
    exp = sl.planes(x, taps, R, M, 48, [0, T, 2 * T, 3 * T])
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ctx = m17hip.Context(FEED_C, T)
    try:
        ctx.wide_raster(FEED_S, R, M, wl.IQ_I16, taps)
        ctx.wide_raster_channels(gr.FEED_SRC, gr.FEED_BINS)
        ctx.reset()
        ctx.wide_survey(48)
        ctx.upload_wide_device_async(dev.data_ptr(), FEED_C, T, W)
        ctx.run(channels=FEED_C, samples=T)
        ctx.upload_wide_device_async(dev.data_ptr() + T * R * sb, FEED_C, T, W)
        _expect_plane(ctx, FEED_S, M, exp[1], "B, behind A's queued run", back=0)
        _expect_plane(ctx, FEED_S, M, exp[0], "A, behind its queued run and B's staging", back=1)
        ctx.run(channels=FEED_C, samples=T)
        ctx.frames()
        ctx.upload_wide_device(dev.data_ptr() + 2 * T * R * sb, FEED_C, T, W)
        _expect_plane(ctx, FEED_S, M, exp[2], "the third block")
        _expect_plane(ctx, FEED_S, M, exp[1], "B, now the block before", back=1)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 3: the survey disturbs nothing -----------------------------------------------------------------------------------------------------------------
def test_the_channels_floats_are_the_same_words_with_the_survey_on_and_off():
    x, taps = gr._feed_case(seed=6350)
    R, M = FEED_R, FEED_M
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    ref = rl.Feeds(x, taps, R, M, gr.FEED_SRC, gr.FEED_BINS, gr.FEED_GAIN)
    want = [ref.block(a, b) for a, b in zip(FEED_CUTS[:-1], FEED_CUTS[1:])]
    ctx = m17hip.Context(FEED_C, max(FEED_LENS))
    try:
        ctx.wide_raster(FEED_S, R, M, wl.IQ_I16, taps)
        ctx.wide_raster_channels(gr.FEED_SRC, gr.FEED_BINS)
        got = {}
        for stride in (0, 5):
            ctx.reset()
            ctx.wide_survey(stride)
            got[stride] = []
            for a, b in zip(FEED_CUTS[:-1], FEED_CUTS[1:]):
                ctx.upload_wide_device(dev.data_ptr() + a * R * sb, FEED_C, b - a, W, gr.FEED_GAIN)
                got[stride].append(ctx.download_f32().copy())
        for k, e in enumerate(want):
            _assert_words(got[0][k], e, ("off", k))
            assert np.array_equal(_u32(got[5][k]), _u32(got[0][k])), k
    finally:
        ctx.close()


def test_a_whole_chain_run_gives_the_same_records_and_diagnostics_with_the_survey_on():
    """One transmission on bin 1 of a 2.4 MSPS source through the whole chain, with the survey off and at stride 48: byte-identical records and m17_diag —
    and the survey, beside that run, finds the bin."""
    R, M = gr.CH_R, gr.CH_M
    bb = ol.generate(ol.gen_params(seed=1, kind=1, lead_in=9600, n_frames=6, tail=4800))
    x = wl.wideband([bb], [12500.0], R, amplitude=6000.0, sigma=gr.CH_SIGMA, seed=1, fmt=wl.IQ_I16)[None]
    T = x.shape[1] // R
    dev = _dev(x)
    out = {}
    for stride in (0, 48):   # (a context each: both runs begin a context's stream)
        ctx = m17hip.Context(1, T)
        try:
            ctx.wide_raster(1, R, M)
            ctx.wide_raster_channels([0], [1])
            ctx.reset()
            ctx.wide_survey(stride)
            ctx.upload_wide_device(dev.data_ptr(), 1, T, x.shape[1])
            ctx.run()
            recs = ctx.frames().copy()
            d = ctx.diag(1)
            out[stride] = (recs.tobytes(), {f: np.array(d[f]).tobytes() for f in tuple(g1.INT_FIELDS) + tuple(g1.FLOAT_FIELDS)})
            if stride:
                power, times, first = ctx.wide_survey_fetch()
                assert times == T // 48 and first == 0
                found = m17hip.wide_raster_occupied(power, 20.0)
                assert found and found[0][:2] == (0, 1)
        finally:
            ctx.close()
    assert len(out[0][0]) > 0 and out[0] == out[48]


# ---- 4: state rules, refusals, timers, memory ---------------------------------------------------------------------------------------------------------
def test_state_rules_refusals_timers_and_memory():
    M, R, L, T, S = 12, 4, 5, 64, 2
    rng = np.random.default_rng(6360)
    x = _data(wl.IQ_I16, S, 3 * T * R, rng)
    dev = _dev(x)
    sb, W = SB[wl.IQ_I16], x.shape[1]
    taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    ctx = m17hip.Context(2, T)

    def up(k, staged=False):
        name = "m17hip_upload_wide_device_async" if staged else "m17hip_upload_wide_device"
        assert _raw(ctx, name, dev.data_ptr() + k * T * R * sb, 2, T, W) == 0
        ctx.C, ctx.T = 2, T

    try:
        ctx.timing(True)
        # before any configuration and under each tuner
        assert _survey(ctx, 1) == ESTATE
        ctx.wide_config(S, R, wl.IQ_I16)
        assert _survey(ctx, 1) == ESTATE and _fetch(ctx, S, M)[0] == ESTATE
        ctx.wide_config2(S, R, 2, wl.IQ_I16)
        assert _survey(ctx, 1) == ESTATE and _fetch(ctx, S, M)[0] == ESTATE
        # under a raster: off is the default
        ctx.wide_raster(S, R, M, wl.IQ_I16, taps)
        ctx.wide_raster_channels([0, 1], [0, -6])
        ctx.reset()
        assert _fetch(ctx, S, M)[0] == ESTATE
        up(0)
        up(1)
        assert _fetch(ctx, S, M)[0] == ESTATE
        assert ctx.timing_get("survey")[1] == 0 and ctx.timing_get("channelise")[1] == 2
        before = ctx.iq_bytes()
        # on: from the next block
        assert _survey(ctx, 4097) == EINVAL and _survey(ctx, 0) == 0 and _survey(ctx, 4096) == 0 and _survey(ctx, 3) == 0
        assert _fetch(ctx, S, M)[0] == ESTATE   # (no block since it was turned on)
        up(2)
        ref = sl.planes(x[:, 2 * T * R:], taps, R, M, 3, [0, T])   # (the device's feed stands at output 2 T: count mod M and N0 follow)
        code, got, t, n0 = _fetch(ctx, S, M)
        assert code == 0 and n0 == 2 * T and t == (3 * T) // 3 - (2 * T) // 3
        feeds = [sl.Survey(taps, R, M, 3) for _ in range(S)]
        for s, f in enumerate(feeds):
            f.block(x[s][: 2 * T * R])
        e2 = np.stack([f.block(x[s][2 * T * R:])[0] for s, f in enumerate(feeds)])
        _assert_words(got, e2, "the first surveyed block, behind two that were not")
        assert not np.array_equal(_u32(e2), _u32(ref[0][0]))   # (the history in front of it counts)
        assert _fetch(ctx, S, M, back=1)[0] == ESTATE          # (one surveyed block only)
        assert ctx.iq_bytes() >= before + 4 * (2 * S * M + S * M * -(-t // 16))
        assert ctx.timing_get("survey")[1] == 1 and ctx.timing_get("channelise")[1] == 3
        # refusals write nothing
        for kw in ({"back": 2}, {"capacity": S * M - 1}, {"null": True}):
            code, buf, t_, n0_ = _fetch(ctx, S, M, **kw)
            assert code == EINVAL and (buf == 7.0).all() and t_ == 0xFFFFFFFF and n0_ == 0xFFFFFFFFFFFFFFFF, kw
        assert ctx.lib.m17hip_wide_survey_fetch(ctx.h, C.c_uint32(0), ol._p(got), C.c_uint64(got.size), None, None) == 0
        # between m17hip_demod_front and its run
        ctx.reset()
        assert _fetch(ctx, S, M)[0] == ESTATE   # (m17hip_demod_reset starts the feeds over: both planes are gone; the survey stays on)
        up(0, staged=True)
        ctx.front(channels=2, samples=T)
        assert _survey(ctx, 5) == ESTATE
        ctx.run(channels=2, samples=T)
        e0 = sl.planes(x, taps, R, M, 3, [0, T])[0]
        _expect_plane(ctx, S, M, e0, "after the reset, staged")
        assert ctx.timing_get("survey")[1] == 2 and ctx.timing_get("channelise")[1] == 4
        # off again, and a configuration call turns it off
        assert _survey(ctx, 0) == 0 and _fetch(ctx, S, M)[0] == ESTATE
        assert _survey(ctx, 2) == 0
        ctx.wide_raster(S, R, M, wl.IQ_I16, taps)
        assert _fetch(ctx, S, M)[0] == ESTATE
        ctx.reset()
        up(1)
        assert _fetch(ctx, S, M)[0] == ESTATE
        assert ctx.timing_get("survey")[1] == 2 and ctx.timing_get("channelise")[1] == 5
        with pytest.raises(m17hip.M17HipError):
            ctx.wide_survey_fetch()
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 5: the example ------------------------------------------------------------------------------------------------------------------------------------
def test_example_scans_beside_the_demodulation():
    """examples/m17-demod-gpu --wide-i16 --decim 50 --raster 192 --bin 1 --scan 48 on the three transmissions of tests/test_gpu_raster_input.py: the frame
    callbacks on stdout are those without --scan, and stderr names bins -61, 1 and 2 — with their offsets in Hz — and no other, block after block."""
    import os
    import re
    import subprocess
    import iq_lib as iq
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in gr.CH_KINDS]
    x = wl.wideband(bb, [12500.0 * b for b in gr.CH_BINS], gr.CH_R, amplitude=6000.0, sigma=gr.CH_SIGMA, seed=1, fmt=wl.IQ_I16)
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    base = [exe, "--wide-i16", "--decim", "50", "--raster", "192", "--bin", "1"]
    raw = np.ascontiguousarray(x).tobytes()
    plain = subprocess.run(base, input=raw, capture_output=True, check=True, timeout=120)
    scan = subprocess.run(base + ["--scan", "48"], input=raw, capture_output=True, check=True, timeout=120)
    assert scan.stdout == plain.stdout and len(plain.stdout.split(b"\n")) >= 6
    found = re.findall(r"scan: bin (-?\d+) ([-+][\d.]+) Hz ([\d.]+) dB", scan.stderr.decode())
    assert {int(b) for b, _, _ in found} == set(gr.CH_BINS), scan.stderr.decode()[-2000:]
    assert all(float(hz) == 12500.0 * int(b) and float(db) > 20.0 for b, hz, db in found)
    assert b"scan: outputs from 0," in scan.stderr
    assert subprocess.run(base[:1] + ["--scan", "48"], input=b"", capture_output=True).returncode == 2   # (--scan goes with --raster)
