"""GPU: K5 (demod_wave_kernel) and kalman_kernel against the RECORDED output of the reference's own demodulator, without the oracle in between.

tests/golden/ref_demod_vectors.npz holds what mobilinkd::M17Demodulator<float> — the reference's text, compiled as it lies over the blaze stand-in of
oracle/blaze_min — delivered on the rows of ref_demod_lib.FIXTURE_CHANNELS under evaluation orders 0 and 3: every frame callback, every diagnostic
callback, and the clock-recovery and deviation-estimator traces.  The rows are regenerated from their arguments and their SHA-256 checked first (a
different row fails).  One batch of 59 channels x 96 000 samples; records byte for byte, the ten callback arguments word for word; no tolerance."""
import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import ref_demod_lib as rl

pytestmark = pytest.mark.gpu

ARGS = ("dcd", "evm", "deviation", "offset", "locked", "clock", "sample_index", "sync_index", "clock_index", "viterbi_cost")   # of the diagnostic callback
ROOM = rl.FIX_T // 384 + 2
DEFAULTS = {3: 48000, 33: -1, 15: 1, 17: 1, 9: 0}
SCHEDULES = {"one_run": {}, "segments_of_1920": {3: 1920, 33: 0}, "staged_two_runs": {}, "deferred_decode_evm_in_k5": {15: 1, 17: 0}}


@pytest.fixture(scope="module")
def fx():
    z = rl.load_fixture()
    x, pol = rl.fixture_rows()
    return z, x, pol


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(64, rl.FIX_T)
    yield c
    c.close()


def _args_equal(got, exp):
    """The ten callback arguments, n_diag and the position (pad) of diagnostic records: every field as raw bytes."""
    return all(got[f].tobytes() == exp[f].tobytes() for f in ARGS + ("n_diag", "pad"))


def _check_records(got, z, order, lo, hi, total, what):
    """Fetched records with lo <= sample_pos < hi against the recorded callbacks.  channel, seq, sync_type and flags are no arguments of the reference's
    callback: they are checked against the device's own count (channels ascending, seq counting per channel from the start of the stream, a sync type
    there is) and then put as the file has them."""
    n = len(rl.FIXTURE_CHANNELS)
    assert got.size == total, (what, got.size, total)
    assert (np.diff(got["channel"].astype(np.int64)) >= 0).all() and (got["channel"] < n).all(), what
    assert (got["sync_type"] <= 3).all(), what
    for c in range(n):
        exp, _ = rl.fixture_channel(z, order, c)
        first = int((exp["sample_pos"] < lo).sum())
        exp = exp[(exp["sample_pos"] >= lo) & (exp["sample_pos"] < hi)]
        g = got[got["channel"] == c].copy()
        assert np.array_equal(g["seq"], first + np.arange(g.size)), (what, rl.FIXTURE_CHANNELS[c])
        g["channel"] = 0
        g["sync_type"] = 0
        g["flags"] = 0
        assert g.tobytes() == exp.tobytes(), (what, rl.FIXTURE_CHANNELS[c], g.size, exp.size)


def _check_log(glog, z, order, lo, hi, what):
    for c, g in enumerate(glog):
        _, exp = rl.fixture_channel(z, order, c)
        pos = exp["pad"][:, 0].astype(np.int64)
        exp = exp[(pos >= lo) & (pos < hi)]
        assert g.size == exp.size and _args_equal(g, exp), (what, rl.FIXTURE_CHANNELS[c], g.size, exp.size)


def _check_final(ctx, z, order, what):
    d = ctx.diag(len(rl.FIXTURE_CHANNELS))
    exp = z[f"last_diag_o{order}"].view(ol.DIAG).reshape(-1)
    for f in ARGS + ("n_diag",):
        bad = np.flatnonzero([d[f][c].tobytes() != exp[f][c].tobytes() for c in range(d.size)])
        assert bad.size == 0, (what, f, [rl.FIXTURE_CHANNELS[c] for c in bad[:8]])


def _total(z, order, lo, hi):
    pos = z[f"recs_o{order}"].view(ol.FRAME_REC).reshape(-1)["sample_pos"]
    return int(((pos >= lo) & (pos < hi)).sum())


def _one_run(ctx, xx, z, order, what):
    ctx.reset()
    ctx.upload(xx)
    ctx.run()
    T = rl.FIX_T
    assert ctx.frames_count() == _total(z, order, 0, T)
    _check_records(ctx.frames(), z, order, 0, T, _total(z, order, 0, T), what)
    _check_log(ctx.diag_log(xx.shape[0], capacity=ROOM), z, order, 0, T, what)
    _check_final(ctx, z, order, what)


def _staged(ctx, x, z, order, what):
    """Two runs of 48 000 samples staged from pinned memory, the second run's front end queued before the first run's results are fetched."""
    import torch
    n, L = x.shape[0], rl.FIX_T // 2
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, k * L:(k + 1) * L])).pin_memory() for k in range(2)]
    ctx.reset()
    ctx.upload_async(pins[0].data_ptr(), n, L)
    ctx.run(channels=n, samples=L)
    ctx.upload_async(pins[1].data_ptr(), n, L)
    ctx.front(channels=n, samples=L)
    try:
        _check_records(ctx.frames(), z, order, 0, L, _total(z, order, 0, L), what + ", run 0")
        _check_log(ctx.diag_log(n, capacity=ROOM), z, order, 0, L, what + ", run 0")
    finally:
        ctx.run(channels=n, samples=L)
        ctx.upload_wait()
    _check_records(ctx.frames(), z, order, L, 2 * L, _total(z, order, L, 2 * L), what + ", run 1")
    _check_log(ctx.diag_log(n, capacity=ROOM), z, order, L, 2 * L, what + ", run 1")
    _check_final(ctx, z, order, what)


@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_the_device_delivers_what_the_references_demodulator_delivered(ctx, fx, schedule, order):
    """One run; segments of 1920; two staged runs with the front end queued first; the decode deferred with the EVM folded inside K5."""
    z, x, pol = fx
    keys = dict(SCHEDULES[schedule])
    keys[9] = ROOM
    what = f"{schedule}, order {order}"
    ctx.set_kalman_order(order)
    ctx.set_channel_polarity(pol)
    for k, v in keys.items():
        ctx.tune(k, v)
    try:
        if schedule == "staged_two_runs":
            _staged(ctx, x, z, order, what)
        else:
            _one_run(ctx, x, z, order, what)
    finally:
        ctx.reset()
        ctx.set_kalman_order(3)
        ctx.set_channel_polarity(None)
        for k in keys:
            ctx.tune(k, DEFAULTS[k])


@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
def test_float_input_delivers_the_same(ctx, fx, order):
    """The same rows as a float stream: the floats the reference was fed (ol.scale of each row under its polarity), no polarity table."""
    z, x, pol = fx
    xf = np.stack([ol.scale(x[c], invert=int(pol[c])) for c in range(x.shape[0])])
    ctx.set_kalman_order(order)
    ctx.tune(9, ROOM)
    try:
        _one_run(ctx, xf, z, order, f"float32, order {order}")
    finally:
        ctx.reset()
        ctx.set_kalman_order(3)
        ctx.tune(9, 0)


@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
def test_kalman_kernel_against_the_recorded_traces(ctx, fx, order):
    """m17hip_kalman_trace, three rows (the last wave ragged), against what the reference's ClockRecovery and FreqDevEstimator were recorded to give:
    the index filter's x and P after every update(index), and idev / offset / deviation recomputed from the two level filters' states."""
    z = fx[0]
    try:
        seqs = rl.clock_sequences()
        calls = [rl.kalman_calls(seqs[j]) for j in rl.DEVICE_CLOCK_ROWS]
        assert all(len(c) == 1 and c[0][0] == 4.0 and c[0][2].size == 100 for c in calls)
        got = ctx.kalman_trace(np.stack([c[0][2] for c in calls]), np.stack([c[0][3] for c in calls]), 10, z0=4.0, order=order)
        for r, j in enumerate(rl.DEVICE_CLOCK_ROWS):
            exp = z[f"clock_o{order}_{len(seqs) + j}"]
            assert rl.same_bits(np.ascontiguousarray(got[r]), np.ascontiguousarray(exp[calls[r][0][1], 3:9])), (order, r)
            assert rl.same_bits(np.ascontiguousarray(got[r, :, 1]), np.ascontiguousarray(exp[calls[r][0][1], 1])), (order, r)      # clock_estimate()
        rows = [rl.dev_sequences()[j] for j in rl.DEVICE_DEV_ROWS]
        mn, mx = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        d192 = np.full((3, mn.shape[1] - 1), 192, dtype=np.uint32)
        lo = ctx.kalman_trace(mn[:, 1:], d192, 0, z0=float(mn[0, 0]), order=order)[..., 0]
        hi = ctx.kalman_trace(mx[:, 1:], d192, 0, z0=float(mx[0, 0]), order=order)[..., 0]
        offset = ((hi + lo).astype(np.float64) / 2.0).astype(np.float32)
        idev = (6.0 / (hi - lo).astype(np.float64)).astype(np.float32)
        for r, j in enumerate(rl.DEVICE_DEV_ROWS):
            exp = z[f"dev_o{order}_{j}"]
            assert np.isfinite(exp).all()
            assert rl.same_bits(idev[r], np.ascontiguousarray(exp[1:, 0])) and rl.same_bits(offset[r], np.ascontiguousarray(exp[1:, 1])), (order, r)
            assert rl.same_bits((np.float32(2400.0) / idev[r]).astype(np.float32), np.ascontiguousarray(exp[1:, 2])), (order, r)
    finally:
        ctx.set_kalman_order(3)
