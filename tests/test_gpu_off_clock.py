"""GPU: transmitters whose symbol clock is off (tests/off_clock.py).  Every other input of the suite has exactly 10 samples per symbol, so the
receiver's clock estimate stays near zero and sample_index hardly ever moves; here it moves 20 to 90 times per channel and run, and the
fastest transmitters make the demodulator lose and regain sync.  What that exercises is the sequential kernel's speculation about the clock
(m17_wave_kernel.hpp: the frame chunk's check that no anti-phase update moves sample_index, its general form, the pending update served inside
a chunk, the index-0 walk of LSF_SYNC) and the 2 x 2 Kalman arithmetic with a second state of 5e-4 instead of 1e-7.

Everything is compared with the oracle bit for bit, no tolerance anywhere: records as bytes, every integer and float field of m17_diag, and —
what pins WHEN sample_index moved — every callback of the diagnostic log.  tests/test_off_clock.py asserts on the oracle alone that these very
inputs do move the clock and still decode."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import off_clock as oc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

INT_FIELDS = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock", "dcd_level")
Cn, T = oc.MAIN_C, oc.MAIN_T
ROOM = T // 384 + 2


# the three configurations of tests/test_gpu_parity.py's ctx fixture (keys 15, 10, 20, 17)
@pytest.fixture(scope="module", params=[(1, -1, 0, 1), (0, -1, 0, 0), (1, 1, 1, 1)], ids=["default", "decode_and_evm_in_k5", "k3_latency_form_redo_in_front"])
def cfg(request):
    return request.param


def _open(cfg, channels=Cn, samples=T):
    c = m17hip.Context(channels, samples)
    for key, v in zip((15, 10, 20, 17), cfg):
        c.tune(key, v)
    return c


@pytest.fixture(scope="module")
def ctx(cfg):
    c = _open(cfg)
    yield c
    c.close()


def _sorted(parts):
    got = np.concatenate(parts)
    return got[np.lexsort((got["seq"], got["channel"]))]


def _check(got, d, rows, diags, what, glog=None, logs=None):
    e = np.concatenate(rows)
    if got.tobytes() != e.tobytes():
        bad = [c for c in range(len(rows)) if got[got["channel"] == c].tobytes() != rows[c].tobytes()]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {e.size} expected), channels {bad[:24]}")
    for f in INT_FIELDS:
        assert np.array_equal(d[f], diags[f]), (what, f, np.flatnonzero(d[f] != diags[f])[:16].tolist())
    for f in FLOAT_FIELDS:
        same = (d[f].view(np.uint32) == diags[f].view(np.uint32)) | (np.isnan(d[f]) & np.isnan(diags[f]))
        assert same.all(), (what, f, np.flatnonzero(~same)[:16].tolist())
    if glog is not None:
        for c in range(len(rows)):
            if glog[c].tobytes() != logs[c].tobytes():
                n = min(glog[c].size, logs[c].size)
                k = next((i for i in range(n) if glog[c][i].tobytes() != logs[c][i].tobytes()), n)
                raise AssertionError(f"{what}: diagnostic log of channel {c} differs at callback {k} of {glog[c].size} / {logs[c].size}: "
                                     f"{glog[c][k] if k < glog[c].size else None} / {logs[c][k] if k < logs[c].size else None}")


def _main():
    x = oc.main()["x"]
    return (x,) + oc.oracle_of("main", x, None, logs=True)


def _chunked(ctx, x, lengths, log=False):
    """The stream as consecutive in-place runs of the given lengths; the records in order, m17_diag after the last run, the runs' logs joined."""
    ctx.reset()
    parts, pos = [], 0
    logs = [[] for _ in range(x.shape[0])]
    for n in lengths:
        ctx.upload(x[:, pos:pos + n])
        ctx.run()
        parts.append(ctx.frames().copy())
        if log:
            for c, lg in enumerate(ctx.diag_log(x.shape[0], capacity=n // 384 + 2)):
                logs[c].append(lg.copy())
        pos += n
    assert pos == x.shape[1]
    return _sorted(parts), ctx.diag(x.shape[0]), [np.concatenate(l) for l in logs] if log else None


# ---- one run ---------------------------------------------------------------------------------------------------------------------------------
def test_one_run_records_diagnostics_and_every_callback(ctx):
    """64 channels x 96 000 samples, kinds 0 / 1 / 2 / 4, noise 0 / 300 / 1200, every ppm of the grid on 4 or 5 channels: records, m17_diag and
    the whole diagnostic log of EVERY channel."""
    x, rows, diags, logs = _main()
    ctx.tune(9, ROOM)
    try:
        ctx.upload(x); ctx.reset(); ctx.run()
        got, d, glog = ctx.frames().copy(), ctx.diag(Cn), ctx.diag_log(Cn, capacity=ROOM)
    finally:
        ctx.tune(9, 0)
    assert got.size > 20 * Cn
    _check(got, d, rows, diags, "one run", glog, logs)


# ---- boundaries: a clock update or a move that falls on a run or segment boundary ---------------------------------------------------------------
def test_ragged_chunks(ctx):
    """The chunk lengths of tests/test_gpu_parity.py::test_full_chain_ragged_chunks."""
    x, rows, diags, logs = _main()
    lengths, pos = [], 0
    for n in (1, 7, 149, 1919, 3841, 9601, 12345, 5000, T):
        n = min(n, T - pos)
        lengths.append(n); pos += n
    got, d, _ = _chunked(ctx, x, lengths)
    _check(got, d, rows, diags, "ragged chunks")


@pytest.mark.parametrize("seg", [0, 7001, 19200])
def test_run_in_segments(ctx, seg):
    x, rows, diags, logs = _main()
    ctx.tune(3, seg)
    ctx.tune(9, ROOM)
    try:
        ctx.upload(x); ctx.reset(); ctx.run()
        got, d, glog = ctx.frames().copy(), ctx.diag(Cn), ctx.diag_log(Cn, capacity=ROOM)
    finally:
        ctx.tune(3, 48000)
        ctx.tune(9, 0)
    _check(got, d, rows, diags, f"segments of {seg}", glog, logs)


def test_chunks_of_a_frame_and_seven_samples(ctx):
    """Runs of 1920 + 7 samples: the run boundary moves seven samples through the frame with every run while the clock drifts, so the 49 runs over
    96 000 samples meet 49 of a frame's 1920 phases (every phase: tests/test_gpu_boundary_phases.py); every run's diagnostic log."""
    x, rows, diags, logs = _main()
    lengths = [1927] * (T // 1927) + ([T % 1927] if T % 1927 else [])
    ctx.tune(9, 8)
    try:
        got, d, glog = _chunked(ctx, x, lengths, log=True)
    finally:
        ctx.tune(9, 0)
    _check(got, d, rows, diags, "chunks of 1927", glog, logs)


# ---- pipelined: staged uploads, the next run's front end queued while the state-machine half of this one works ------------------------------------
@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
def test_pipelined_staged_runs(ctx, order):
    """The call sequence of tests/test_gpu_streaming.py's _pipelined, both call orders, five runs of 19 200 samples."""
    import torch
    x, rows, diags, logs = _main()
    n, L = 5, T // 5
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, k * L:(k + 1) * L])).pin_memory() for k in range(n)]
    ctx.reset()
    ctx.upload_async(pins[0].data_ptr(), Cn, L)
    ctx.run(channels=Cn, samples=L)
    parts = []
    for k in range(n):
        if k + 1 < n:
            ctx.upload_async(pins[k + 1].data_ptr(), Cn, L)
            ctx.front(channels=Cn, samples=L)
            if order == "run_then_fetch":
                ctx.run(channels=Cn, samples=L)
                ctx.frames_select(1)
        parts.append(ctx.frames().copy())
        ctx.frames_select(0)
        if k + 1 < n and order != "run_then_fetch":
            ctx.run(channels=Cn, samples=L)
    ctx.upload_wait()
    _check(_sorted(parts), ctx.diag(Cn), rows, diags, f"pipelined, {order}")


# ---- every evaluation order of the 2 x 2 Kalman arithmetic -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", oc.KALMAN_ORDERS)
def test_each_kalman_order(ctx, order):
    """The first 32 channels x 48 000 samples under each order (tests/test_gpu_kalman.py's pattern).  Off the clock the orders do end with
    different clock estimates (tests/test_off_clock.py), so an order the kernel gets wrong shows."""
    x = np.ascontiguousarray(oc.main()["x"][:32, :48000])
    lib = ol.oracle()
    lib.m17o_set_kalman_order(C.c_int(order))
    try:
        recs, counts, diags = ol.demod_batch(x, cap=2 * (48000 // 1920 + 2) + 4, threads=oc.THREADS)
        logs = oc.par(lambda c: oc.demod_log(x[c]), range(32))
    finally:
        lib.m17o_set_kalman_order(C.c_int(3))
    rows = [recs[c, :counts[c]] for c in range(32)]
    ctx.set_kalman_order(order)
    ctx.tune(9, ROOM)
    try:
        ctx.upload(x); ctx.reset(); ctx.run()
        got, d, glog = ctx.frames().copy(), ctx.diag(32), ctx.diag_log(32, capacity=ROOM)
    finally:
        ctx.set_kalman_order(3)
        ctx.tune(9, 0)
    assert got.size > 10 * 32
    _check(got, d, rows, diags, f"order {order}", glog, logs)
    assert np.array_equal(d["pad"], diags["pad"])   # live clock / sync counters at the end of the run


# ---- with the per-channel features -----------------------------------------------------------------------------------------------------------
def test_mixed_channel_polarity(cfg):
    """A mixed m17hip_set_channel_polarity table; the channels it inverts come from inverted transmitters."""
    x, pol = oc.main_mixed_polarity()
    rows, diags, logs = oc.oracle_of("mixed polarity", x, pol, logs=True)
    c = _open(cfg)
    try:
        c.set_channel_polarity(pol)
        c.tune(9, ROOM)
        c.upload(x); c.reset(); c.run()
        _check(c.frames().copy(), c.diag(Cn), rows, diags, "mixed polarity", c.diag_log(Cn, capacity=ROOM), logs)
    finally:
        c.close()


def test_reset_channels_between_two_runs_of_drifting_streams(cfg):
    """Two runs of 48 000 samples, fresh demodulators for oc.RESET_CHANNELS in front of the second: a reset channel reports what a fresh oracle
    demodulator started at sample 48 000 reports (records, m17_diag, every callback), its neighbours what the oracle reports over the whole
    stream — they keep their clock state."""
    x, rows, diags, logs = _main()
    half = T // 2
    rs = list(oc.RESET_CHANNELS)
    frows, fdiags, flogs = oc.oracle_of("reset fresh", x[rs, half:], None, logs=True)
    exp_rows, exp_diags, exp_logs = [], diags.copy(), []
    for c in range(Cn):
        if c in rs:
            i = rs.index(c)
            r = frows[i].copy(); r["channel"] = c
            exp_rows.append(r); exp_diags[c] = fdiags[i]; exp_logs.append(flogs[i])
        else:
            exp_rows.append(rows[c][rows[c]["sample_pos"] >= half])
            exp_logs.append(logs[c][oc.log_pos(logs[c]) >= half])
    first_rows = [r[r["sample_pos"] < half] for r in rows]
    first_logs = [l[oc.log_pos(l) < half] for l in logs]
    c = _open(cfg)
    try:
        c.tune(9, ROOM)
        c.reset()
        c.upload(x[:, :half]); c.run()
        got0, glog0 = c.frames().copy(), c.diag_log(Cn, capacity=ROOM)
        c.reset_channels(rs)
        c.upload(x[:, half:]); c.run()
        got1, d1, glog1 = c.frames().copy(), c.diag(Cn), c.diag_log(Cn, capacity=ROOM)
    finally:
        c.close()
    assert got0.tobytes() == np.concatenate(first_rows).tobytes()
    for ch in range(Cn):
        assert glog0[ch].tobytes() == first_logs[ch].tobytes(), ("first run, diagnostic log", ch)
    _check(got1, d1, exp_rows, exp_diags, "second run", glog1, exp_logs)


# ---- gate-aware front end ----------------------------------------------------------------------------------------------------------------------
def test_gate_aware_front_end_on_bursty_drifting_channels(cfg):
    """m17hip_tune key 26 = 1 in segments of 4800 samples (tests/test_gpu_parity.py::test_gate_aware_front_end_on_bursty_channels), every burst
    +500 or -500 ppm off: the oracle's records and diagnostics, and the same with the gate-aware path off."""
    x, _ = oc.bursty()
    rows, diags, logs = oc.oracle_of("bursty", x, None, logs=True)
    n = x.shape[0]
    c = _open(cfg, n, x.shape[1])
    try:
        c.tune(3, 4800)
        c.tune(9, ROOM)
        outs = []
        for mode in (1, 0):
            c.tune(26, mode)
            c.upload(x); c.reset(); c.run()
            got = c.frames().copy()
            _check(got, c.diag(n), rows, diags, f"bursty, gate-aware {mode}", c.diag_log(n, capacity=ROOM), logs)
            outs.append(got.tobytes())
        assert outs[0] == outs[1]
    finally:
        c.close()


# ---- random scenarios --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", oc.SCENARIO_SEEDS)
def test_random_scenarios_resampled(ctx, seed):
    """oracle_lib.random_scenario (all five kinds back to back, lost sync, forced unlocks, silence), 32 channels, each re-read at a ppm drawn
    from the grid; run in 19 200-sample segments as tests/test_gpu_parity.py::test_full_chain_random_scenarios."""
    x, _ = oc.scenarios(seed, 32)
    rows, diags, logs = oc.oracle_of(("scenarios", seed), x, None, logs=True)
    ctx.tune(3, 19200)
    ctx.tune(9, ROOM)
    try:
        ctx.upload(x); ctx.reset(); ctx.run()
        got, d, glog = ctx.frames().copy(), ctx.diag(32), ctx.diag_log(32, capacity=ROOM)
    finally:
        ctx.tune(3, 48000)
        ctx.tune(9, 0)
    _check(got, d, rows, diags, f"scenarios {seed}", glog, logs)
