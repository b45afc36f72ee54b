"""GPU tests of the source spectrum (ABI 616, include/m17hip.h: m17hip_wide_spectrum): spectrum_kernel windows and transforms every frame of every source
block and sums the powers per group of 16 frames, chan_survey_sum_kernel adds the groups.  Every comparison is exact: the plane
(m17hip_wide_spectrum_fetch) as uint32 words against the HOST form of the same arithmetic (tests/spectrum_lib.py: detail/core.h under the host compiler)
— NaN-ness where that is a NaN.  What the host form itself is worth is asserted without a GPU in tests/test_spectrum.py.  The helpers of
tests/test_gpu_wide_input.py and tests/test_gpu_raster_input.py are imported as they stand."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import spectrum_lib as sp
import test_gpu_raster_input as gr
import test_gpu_wide_input as g1
import wide_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
FMTS, SB = g1.FMTS, g1.SB
_data, _dev, _raw = gr._data, gr._dev, gr._raw
_u32, _assert_words = g1._u32, g1._assert_words
NAMES = ("m17hip_upload_wide", "m17hip_upload_wide_async", "m17hip_upload_wide_device", "m17hip_upload_wide_device_async")


def _spectrum(ctx, N, hop, win=None, nwin=None):
    w = None if win is None else np.ascontiguousarray(win, dtype=np.float32)
    return ctx.lib.m17hip_wide_spectrum(ctx.h, C.c_uint32(N), C.c_uint32(hop), None if w is None else ol._p(w),
                                        C.c_uint32((0 if w is None else w.size) if nwin is None else nwin))


def _fetch(ctx, S, N, back=0, capacity=None, null=False):
    """(code, plane [S][N], frames, first_sample); the buffer is pre-filled with 7 so that a refusal that writes shows."""
    buf = np.full(S * N, 7.0, dtype=np.float32)
    j, f = C.c_uint32(0xFFFFFFFF), C.c_uint64(0xFFFFFFFFFFFFFFFF)
    code = ctx.lib.m17hip_wide_spectrum_fetch(ctx.h, C.c_uint32(back), None if null else ol._p(buf), C.c_uint64(buf.size if capacity is None else capacity),
                                              C.byref(j), C.byref(f))
    return code, buf.reshape(S, N), j.value, f.value


def _expect_plane(ctx, S, N, exp, what, back=0):
    plane, J, first_sample = exp
    code, got, j, f = _fetch(ctx, S, N, back)
    assert code == 0, (what, code)
    assert (j, f) == (J, first_sample), (what, j, f, J, first_sample)
    _assert_words(got, plane, what)


# The four configurations at their smallest shapes: (outputs per group, source samples per group) and two channels each.
KINDS = {"config": (1, 2), "config2": (1, 4), "raster": (1, 4), "resample": (2, 3)}


def _configure(ctx, kind, S, fmt):
    if kind == "config":
        ctx.wide_config(S, 2, fmt)
    elif kind == "config2":
        ctx.wide_config2(S, 2, 2, fmt)
    elif kind == "raster":
        ctx.wide_raster(S, 4, 48, fmt)
    else:
        ctx.wide_resample(S, 1, 2, 3, fmt)
    if kind == "raster":
        ctx.wide_raster_channels([0, S - 1], [1, -3])
    else:
        ctx.wide_channels([0, S - 1], [m17hip.wide_fcw(7000.0, 2), m17hip.wide_fcw(-11000.0, 2)])
    return KINDS[kind]


def _block(ctx, name, ptr, T, P, run=True):
    """One block of T outputs by any of the four ways in; a staged one is followed by its run."""
    assert _raw(ctx, name, ptr, 2, T, P) == 0, name
    ctx.C, ctx.T = 2, T
    if name.endswith("_async") and run:
        ctx.run(channels=2, samples=T)


# ---- 1: every size ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS), ids=list(FMTS))
@pytest.mark.parametrize("N", (64, 128, 256, 512, 1024, 2048, 4096))
def test_every_size_and_format_against_the_host_form(N, fmt):
    """Three sources under wide_config at decim 2, one block of 17 overlapping frames (hop N / 2 + 3: a group of 16 and a group of one; at N <= 1024 several
    frames per pass and a last pass that is not full), a ramp window of the caller's, rows that are not 16-byte aligned.  In float32 the data hold
    components up to 1e9, denormals and zeroes of either sign."""
    f, S, hop = FMTS[fmt], 3, N // 2 + 3
    W = (16 * hop + N + 3) // 2 * 2
    rng = np.random.default_rng(6170 + N + f)
    host = _data(f, S, W + 3, rng)
    dev = _dev(host)
    win = (0.25 + np.arange(N) / N).astype(np.float32)
    exp = sp.planes([host[s][:W] for s in range(S)], N, hop, [0, W], win)[0]
    assert exp[1] == 17 and exp[2] == 0 and np.isfinite(exp[0]).all() and (exp[0] > 0).all()
    ctx = m17hip.Context(2, W // 2)
    try:
        _configure(ctx, "config", S, f)
        ctx.reset()
        ctx.wide_spectrum(N, hop, win)
        _block(ctx, NAMES[2], dev.data_ptr(), W // 2, W + 3)
        _expect_plane(ctx, S, N, exp, (N, fmt))
        power, frames, first = ctx.wide_spectrum_fetch()
        assert power.shape == (S, N) and power.dtype == np.float32 and (frames, first) == (17, 0)
        _assert_words(power, exp[0], "Context.wide_spectrum_fetch")
    finally:
        ctx.close()


# ---- 2: every configuration, and the spectrum disturbs nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_configuration_and_the_channels_floats_are_the_same_words_on_and_off(kind):
    """Two sources, two channels, three blocks of a feed (the second begins at a count that is no multiple of the hop) with the spectrum off and on at the
    default window: the planes are the host form's, and the float slab the channels get is the same words either way.  Under the raster the survey runs
    beside it, and its planes are the same words too."""
    S, N, hop, f = 2, 64, 50, wl.IQ_I16
    u, g = KINDS[kind]
    groups = (40, 61, 90)
    cuts = np.cumsum((0,) + tuple(k * g for k in groups)).tolist()
    rng = np.random.default_rng(6180 + len(kind))
    x = _data(f, S, cuts[-1], rng)
    dev = _dev(x)
    sb, P = SB[f], x.shape[1]
    exp = sp.planes(x, N, hop, cuts)
    assert all(e[1] > 0 for e in exp) and cuts[1] % hop != 0
    ctx = m17hip.Context(2, max(groups) * u)
    got = {}
    try:
        for on in (False, True):
            _configure(ctx, kind, S, f)
            if kind == "raster":
                ctx.wide_survey(3)
            ctx.reset()
            if on:
                ctx.wide_spectrum(N, hop)
            got[on] = []
            for k, (a, n) in enumerate(zip(cuts[:-1], groups)):
                _block(ctx, NAMES[2], dev.data_ptr() + a * sb, n * u, P)
                slab = ctx.download_f32().copy()
                survey = ctx.wide_survey_fetch()[0] if kind == "raster" else None
                got[on].append((slab, survey))
                if on:
                    _expect_plane(ctx, S, N, exp[k], (kind, k))
                else:
                    assert _fetch(ctx, S, N)[0] == ESTATE
        for (s0, v0), (s1, v1) in zip(got[False], got[True]):
            assert s0.size > 0 and np.array_equal(_u32(s0), _u32(s1)), kind
            assert v0 is None or (v0.size == S * 48 and np.array_equal(_u32(v0), _u32(v1)))
    finally:
        ctx.close()


# ---- 3: frames and hops ------------------------------------------------------------------------------------------------------------------------------------
def test_frame_counts_and_hops():
    """wide_config at decim 1, so a block has any number of samples.  J = 0 (W < N: the plane is all +0 and frames is 0), 1, 16, 17, 33; hop < N, hop > N,
    a hop that does not divide W, hop = 1 at N = 64 with W = 200 (137 frames: nine groups); N = 256 with eight frames per pass and groups whose last pass
    holds one frame."""
    cases = [(64, 64, 63), (64, 64, 64), (64, 64, 16 * 64), (64, 64, 17 * 64 + 9), (64, 64, 33 * 64 + 63), (64, 20, 500), (64, 100, 1000), (64, 1, 200),
             (64, 7, 64), (64, 1 << 24, 100), (256, 100, 256 + 32 * 100 + 50), (128, 128, 17 * 128)]
    S, f = 2, wl.IQ_U8
    rng = np.random.default_rng(6190)
    Wmax = max(c[2] for c in cases)
    host = _data(f, S, Wmax + 1, rng)
    dev = _dev(host)
    ctx = m17hip.Context(2, Wmax)
    seen = set()
    try:
        ctx.wide_config(S, 1, f)
        ctx.wide_channels([0, 1], [1 << 28, -(1 << 29)])
        for N, hop, W in cases:
            exp = sp.planes([host[s][:W] for s in range(S)], N, hop, [0, W])[0]
            assert exp[1] == sp.frames_stated(0, W, N, hop)[1]
            seen.add(exp[1])
            ctx.reset()
            assert _spectrum(ctx, N, hop) == 0
            _block(ctx, NAMES[2], dev.data_ptr(), W, Wmax + 1)
            _expect_plane(ctx, S, N, exp, (N, hop, W))
            if exp[1] == 0:
                assert (_u32(_fetch(ctx, S, N)[1]) == 0).all()
        assert {0, 1, 16, 17, 33, 137} <= seen
    finally:
        ctx.close()


# ---- 4: the feed -------------------------------------------------------------------------------------------------------------------------------------------
def test_a_feed_in_ragged_blocks_by_all_four_ways_in():
    """Blocks of 10, 120, 31, 64, 257, 1 and 900 samples of two sources (wide_config at decim 1) at N = 64, hop = 48, by host, pinned, device and staged
    device memory by turns: `first` follows the feed's count (the blocks begin at 0, 10, 130, 161, 225, 482, 483), *first_sample is reported, blocks without
    a frame have +0 planes, back = 1 is the block before."""
    S, N, hop, f = 2, 64, 48, wl.IQ_I16
    import torch
    lens = (10, 120, 31, 64, 257, 1, 900)
    cuts = np.cumsum((0,) + lens).tolist()
    rng = np.random.default_rng(6200)
    x = _data(f, S, cuts[-1], rng)
    xc = np.ascontiguousarray(x)
    dev, pin = _dev(x), torch.from_numpy(np.array(x)).pin_memory()
    ptrs = dict(zip(NAMES, (xc.ctypes.data, pin.data_ptr(), dev.data_ptr(), dev.data_ptr())))
    sb, P = SB[f], x.shape[1]
    exp = sp.planes(x, N, hop, cuts)
    assert [e[1] for e in exp] == [0, 1, 0, 0, 4, 0, 17] and [e[2] for e in exp] == [0, 48, 144, 192, 240, 528, 528]
    how = [NAMES[2], NAMES[0], NAMES[3], NAMES[1], NAMES[3], NAMES[0], NAMES[1]]
    ctx = m17hip.Context(2, max(lens))
    try:
        ctx.wide_config(S, 1, f)
        ctx.wide_channels([0, 1], [1 << 28, -(1 << 29)])
        ctx.reset()
        ctx.wide_spectrum(N, hop)
        for k, (a, n, h) in enumerate(zip(cuts[:-1], lens, how)):
            _block(ctx, h, ptrs[h] + a * sb, n, P)
            _expect_plane(ctx, S, N, exp[k], (h, a, n))
            if k:
                _expect_plane(ctx, S, N, exp[k - 1], (h, a, n, "the block before"), back=1)
        ctx.upload_wait()
        ctx.frames()
    finally:
        ctx.close()


def test_a_fetch_behind_a_queued_run_and_a_later_staged_block_names_the_right_planes():
    """Block A staged, its run queued, block B staged — and only then the fetches: back = 1 is A's plane, back = 0 is B's.  B's run and a third block in
    place follow, and the planes move on by one."""
    S, N, hop, f, T = 2, 128, 100, wl.IQ_I16, 960
    rng = np.random.default_rng(6210)
    x = _data(f, S, 3 * T, rng)
    dev = _dev(x)
    sb, P = SB[f], x.shape[1]
    exp = sp.planes(x, N, hop, [0, T, 2 * T, 3 * T])
    ctx = m17hip.Context(2, T)
    try:
        ctx.wide_config(S, 1, f)
        ctx.wide_channels([0, 1], [1 << 28, -(1 << 29)])
        ctx.reset()
        ctx.wide_spectrum(N, hop)
        _block(ctx, NAMES[3], dev.data_ptr(), T, P)
        _block(ctx, NAMES[3], dev.data_ptr() + T * sb, T, P, run=False)
        _expect_plane(ctx, S, N, exp[1], "B, behind A's queued run", back=0)
        _expect_plane(ctx, S, N, exp[0], "A, behind its queued run and B's staging", back=1)
        ctx.run(channels=2, samples=T)
        ctx.frames()
        _block(ctx, NAMES[2], dev.data_ptr() + 2 * T * sb, T, P)
        _expect_plane(ctx, S, N, exp[2], "the third block")
        _expect_plane(ctx, S, N, exp[1], "B, now the block before", back=1)
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: non-finite samples ---------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_and_an_infinity_reach_the_frames_that_contain_them_and_no_other_source():
    """Three float32 sources at N = 64, hop = 100 (samples 64..99 of every hundred lie in no frame).  A NaN and an infinity of source 1 BETWEEN frames reach
    nothing; inside frames 0 and 2 they make source 1's plane what the host form says — not finite in any bin — while sources 0 and 2 keep the host
    form's finite words."""
    S, N, hop, W, f = 3, 64, 100, 464, wl.IQ_F32
    rng = np.random.default_rng(6220)
    base = np.array(_data(f, S, W, rng))
    ctx = m17hip.Context(2, W)
    try:
        ctx.wide_config(S, 1, f)
        ctx.wide_channels([0, 2], [1 << 28, -(1 << 29)])
        for where, hit in (((70, 170), False), ((10, 230), True)):
            x = base.copy()
            x[1, where[0]] = complex(np.nan, 1.0)
            x[1, where[1]] = complex(2.0, -np.inf)
            exp = sp.planes(x, N, hop, [0, W])[0]
            assert exp[1] == 5 and np.isfinite(exp[0][[0, 2]]).all() and np.isfinite(exp[0][1]).all() == (not hit)
            assert not hit or not np.isfinite(exp[0][1]).any()
            dev = _dev(x)
            ctx.reset()
            ctx.wide_spectrum(N, hop)
            _block(ctx, NAMES[2], dev.data_ptr(), W, W)
            _expect_plane(ctx, S, N, exp, where)
    finally:
        ctx.close()


# ---- 6: state rules, refusals, timers, memory ------------------------------------------------------------------------------------------------------------------
def test_state_rules_refusals_timers_and_memory():
    S, N, hop, T, f = 2, 64, 32, 256, wl.IQ_I16
    rng = np.random.default_rng(6230)
    x = _data(f, S, 3 * T, rng)
    dev = _dev(x)
    sb, P = SB[f], x.shape[1]
    win = np.linspace(0.5, 1.5, N).astype(np.float32)
    ctx = m17hip.Context(2, T)

    def up(k, staged=False):
        _block(ctx, NAMES[3] if staged else NAMES[2], dev.data_ptr() + k * T * sb, T, P, run=False)

    try:
        ctx.timing(True)
        # before any wideband configuration
        assert _spectrum(ctx, N, hop) == ESTATE and _spectrum(ctx, 0, 0) == ESTATE and _fetch(ctx, S, N)[0] == ESTATE
        ctx.wide_config(S, 1, f)
        ctx.wide_channels([0, 1], [1 << 28, -(1 << 29)])
        ctx.reset()
        # off is the default
        assert _fetch(ctx, S, N)[0] == ESTATE
        up(0)
        assert _fetch(ctx, S, N)[0] == ESTATE and ctx.timing_get("spectrum")[1] == 0 and ctx.timing_get("tune")[1] == 1
        before = ctx.iq_bytes()
        # outside the limits: nothing changes (the spectrum stays off)
        bad = win.copy()
        bad[5] = np.inf
        for args in ((32, hop), (96, hop), (8192, hop), (N, 0), (N, (1 << 24) + 1), (N, hop, win[:-1]), (N, hop, win, N - 1), (N, hop, bad), (N, hop, None, N)):
            assert _spectrum(ctx, *args) == EINVAL, args[:2]
        up(1)
        assert _fetch(ctx, S, N)[0] == ESTATE and ctx.timing_get("spectrum")[1] == 0
        # on: from the next block, at the feed's count
        assert _spectrum(ctx, N, 1 << 24) == 0 and _spectrum(ctx, 4096, 1) == 0 and _spectrum(ctx, N, hop, win) == 0
        assert _fetch(ctx, S, N)[0] == ESTATE   # (no block since it was turned on)
        up(2)
        exp = sp.planes(x, N, hop, [2 * T, 3 * T], win)[0]
        assert exp[2] == 2 * T and exp[1] == (T - N) // hop + 1
        _expect_plane(ctx, S, N, exp, "the first transformed block, behind two that were not")
        assert _fetch(ctx, S, N, back=1)[0] == ESTATE   # (one block only)
        assert ctx.iq_bytes() >= before + 4 * (2 * S * N + S * N * -(-exp[1] // 16) + 2 * N)
        assert ctx.timing_get("spectrum")[1] == 1 and ctx.timing_get("tune")[1] == 3
        # an EINVAL now changes nothing either: the next block is transformed with what held before
        assert _spectrum(ctx, 100, hop) == EINVAL
        # refusals of the fetch write nothing
        for kw in ({"back": 2}, {"capacity": S * N - 1}, {"null": True}):
            code, buf, j_, f_ = _fetch(ctx, S, N, **kw)
            assert code == EINVAL and (buf == 7.0).all() and j_ == 0xFFFFFFFF and f_ == 0xFFFFFFFFFFFFFFFF, kw
        got = np.zeros(S * N, dtype=np.float32)
        assert ctx.lib.m17hip_wide_spectrum_fetch(ctx.h, C.c_uint32(0), ol._p(got), C.c_uint64(got.size), None, None) == 0
        _assert_words(got.reshape(S, N), exp[0], "a fetch without the two counts")
        # m17hip_demod_reset forgets the planes and starts the feed over; between m17hip_demod_front and its run
        ctx.reset()
        assert _fetch(ctx, S, N)[0] == ESTATE
        up(0, staged=True)
        ctx.front(channels=2, samples=T)
        assert _spectrum(ctx, N, hop) == ESTATE and _spectrum(ctx, 0, 0) == ESTATE
        ctx.run(channels=2, samples=T)
        _expect_plane(ctx, S, N, sp.planes(x, N, hop, [0, T], win)[0], "after the reset, staged")
        assert ctx.timing_get("spectrum")[1] == 2
        # a new window travels with the next block; the planes before it are forgotten
        assert _spectrum(ctx, N, hop) == 0 and _fetch(ctx, S, N)[0] == ESTATE
        up(1)
        _expect_plane(ctx, S, N, sp.planes(x, N, hop, [T, 2 * T])[0], "the default window after the caller's")
        # off, and every configuration call turns it off
        assert _spectrum(ctx, 0, 0) == 0 and _fetch(ctx, S, N)[0] == ESTATE
        for cfg in (lambda: ctx.wide_config(S, 1, f), lambda: ctx.wide_config2(S, 1, 1, f), lambda: ctx.wide_raster(S, 1, 4, f),
                    lambda: ctx.wide_resample(S, 1, 1, 1, f)):
            assert _spectrum(ctx, N, hop) == 0
            up(0)
            assert _fetch(ctx, S, N)[0] == 0
            cfg()
            assert _fetch(ctx, S, N)[0] == ESTATE
            ctx.reset()
            n = ctx.timing_get("spectrum")[1]
            up(1)
            assert _fetch(ctx, S, N)[0] == ESTATE and ctx.timing_get("spectrum")[1] == n
        with pytest.raises(m17hip.M17HipError):
            ctx.wide_spectrum_fetch()
        with pytest.raises(m17hip.M17HipError):
            ctx.wide_spectrum_fetch(back=2)
        ctx.timing(False)
    finally:
        ctx.close()


# ---- 7: the workflow -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_finds_the_carriers_the_host_form_finds():
    """The first 0.128 s of tests/test_resample_input.py's 2.048 MSPS source under the resampling tuner at 16 x 3 / 8: the plane at 2048 points is the host
    form's, so wide_spectrum_carriers finds on the device what tests/test_spectrum.py finds on the host — three carriers, within 450 Hz of -762.5, +12.5 and
    +25 kHz."""
    import test_resample_input as tri
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tri.KINDS]
    W = 262144
    x = np.ascontiguousarray(tri.source_2048k(bb)[None, :W])
    N, T = 2048, W // 128 * 3
    exp = sp.planes(x, N, N, [0, W])[0]
    dev = _dev(x)
    ctx = m17hip.Context(2, T)
    try:
        ctx.wide_resample(1, 16, 3, 8)
        ctx.wide_channels([0, 0], [0, 0])
        ctx.reset()
        ctx.wide_spectrum(N, N)
        _block(ctx, NAMES[2], dev.data_ptr(), T, W)
        _expect_plane(ctx, 1, N, exp, "2.048 MSPS")
        found = m17hip.wide_spectrum_carriers(ctx.wide_spectrum_fetch()[0], 2048000.0)
        assert len(found) == 3, found
        for f0 in tri.OFFSETS:
            assert min(abs(hz - f0) for _, hz, _ in found) <= 450.0, (f0, found)
    finally:
        ctx.close()


# ---- 8: the example ------------------------------------------------------------------------------------------------------------------------------------------
def test_example_prints_the_carriers_beside_the_demodulation():
    """examples/m17-demod-gpu --wide-i16 --rate 2048000 --offset-hz 12500 --spectrum 2048 on the same source: the frame callbacks on stdout are those without
    --spectrum, and stderr names, for every full block (1920 outputs: 81 920 samples, 40 frames on the feed's grid), three carriers within 450 Hz of -762.5,
    +12.5 and +25 kHz and no other.  --spectrum goes with a wideband format and a power of two."""
    import os
    import re
    import subprocess
    import iq_lib as iq
    import test_resample_input as tri
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tri.KINDS]
    raw = np.ascontiguousarray(tri.source_2048k(bb)).tobytes()
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    base = [exe, "--wide-i16", "--rate", "2048000", "--offset-hz", "12500"]
    plain = subprocess.run(base, input=raw, capture_output=True, check=True, timeout=120)
    spec = subprocess.run(base + ["--spectrum", "2048"], input=raw, capture_output=True, check=True, timeout=120)
    assert spec.stdout == plain.stdout and len(plain.stdout.split(b"\n")) >= 6
    blocks = re.split(r"spectrum: samples from ", spec.stderr.decode())[1:]
    full = 0
    for k, b in enumerate(blocks):
        first, frames = re.match(r"(\d+), (\d+) frames", b).groups()
        assert int(first) == k * 81920 and int(first) % 2048 == 0
        found = [float(hz) for hz, _ in re.findall(r"spectrum: carrier ([-+][\d.]+) Hz ([\d.]+) dB", b)]
        if int(frames) == 40:
            full += 1
            assert len(found) == 3 and all(min(abs(hz - f0) for hz in found) <= 450.0 for f0 in tri.OFFSETS), (k, found)
    assert full >= 10 and full >= len(blocks) - 1
    for bad in (["--spectrum", "2048"], base + ["--spectrum", "1000"], base + ["--spectrum", "32"], base + ["--spectrum", "64", "--hop", "0"], base + ["--hop", "5"]):
        assert subprocess.run(bad if bad[0] == exe else [exe] + bad, input=b"", capture_output=True).returncode == 2, bad
