"""CPU: the clock-offset helper (tests/off_clock.py) and, on the ORACLE alone, the conditions under which tests/test_gpu_off_clock.py can fail:
its inputs do make the receiver's clock recovery move (sample_index changes in the diagnostic log), the transmissions still decode, and the
fastest transmitters do make the demodulator lose and regain sync.  Also off the clock: the oracle against the orchestrator over the reference's
own operator objects (where oracle/_ref was built)."""
import ctypes as C
import os

import numpy as np
import pytest

import off_clock as oc
import oracle_lib as ol


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------
def test_resample_zero_ppm_is_the_identity():
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, 5000).astype(np.int16)
    x[:40] = 32767
    x[-40:] = -32768
    assert np.array_equal(oc.resample_clock(x, 0), x)
    assert np.array_equal(oc.resample_clock(x, 0.0, half=4), x)
    x2 = np.stack([x, x[::-1]])
    assert np.array_equal(oc.resample_clock(x2, 0), x2)
    assert np.array_equal(oc.resample_clock(x2, [0, 0]), x2)


def test_resample_is_deterministic_per_row_and_saturates():
    rng = np.random.default_rng(2)
    x = rng.integers(-20000, 20000, (3, 4000)).astype(np.int16)
    ppm = [500.0, -500.0, 2000.0]
    a, b = oc.resample_clock(x, ppm), oc.resample_clock(x.copy(), ppm)
    assert a.dtype == np.int16 and a.shape == x.shape and np.array_equal(a, b)
    for r in range(3):                                               # the 2-D form is the 1-D form per row, under that row's ppm
        assert np.array_equal(a[r], oc.resample_clock(x[r], ppm[r]))
        assert not np.array_equal(a[r], x[r])
    assert np.array_equal(oc.resample_clock(x, 500.0)[1], oc.resample_clock(x[1], 500.0))   # a scalar serves every row
    # samples outside the array are 0: at +2000 ppm the last outputs of 40 000 are read 79 samples past the end, beyond the window's reach
    z = oc.resample_clock(np.full(40000, 1000, dtype=np.int16), 2000.0)
    assert (z[-40:] == 0).all() and (np.abs(z[:39000].astype(np.int32) - 1000) <= 5).all()
    # the interpolation of a full-scale alternating signal overshoots: the result saturates, it does not wrap
    s = np.tile(np.array([32767, 32767, -32768, -32768], dtype=np.int16), 500)
    y = oc.resample_clock(s, 800.0).astype(np.int32)
    assert y.max() == 32767 and y.min() == -32768 and (y == 32767).sum() > 100 and (y == -32768).sum() > 100


def test_resample_formula_on_a_few_samples():
    """out[n] against the sum written out in Python floats, term by term."""
    import math
    rng = np.random.default_rng(3)
    x = rng.integers(-30000, 30000, 300).astype(np.int16)
    half, ppm = 16, 1000.0
    y = oc.resample_clock(x, ppm, half)
    for n in (0, 1, 17, 150, 283, 299):
        p = n * (1.0 + ppm * 1e-6)
        i0 = math.floor(p)
        f = p - i0
        acc = 0.0
        for k in range(-half + 1, half + 1):
            d = f - k
            if not 0 <= i0 + k < x.size or abs(d) >= half:
                continue
            sinc = 1.0 if d == 0.0 else math.sin(math.pi * d) / (math.pi * d)
            acc += float(x[i0 + k]) * sinc * 0.5 * (1.0 + math.cos(math.pi * d / half))
        assert abs(int(y[n]) - acc) <= 0.5 + 1e-6, (n, int(y[n]), acc)


def test_a_fast_transmitters_last_sync_word_comes_early_by_the_expected_number_of_samples():
    """A long clean BERT burst at +500 ppm against the same burst on the clock: the oracle's last frame record (its sample_pos) lies earlier by
    pos * 500e-6 / (1 + 500e-6) samples, within one sample."""
    T = 96000
    on, off = oc.burst(79, 0, T, sigma=0.0, ppm=0.0), oc.burst(79, 0, T, sigma=0.0, ppm=500.0)
    r0, _ = ol.demod(on)
    r1, _ = ol.demod(off)
    assert r0.size >= 40 and r1.size >= 40
    # the last frame both report, told by its payload (the PRBS9 sequence never repeats within a burst)
    where = {bytes(r["payload"][:25]): int(r["sample_pos"]) for r in r1}
    last = [r for r in r0 if bytes(r["payload"][:25]) in where][-1]
    p0, p1 = int(last["sample_pos"]), where[bytes(last["payload"][:25])]
    expected = p0 * 500e-6 / (1.0 + 500e-6)
    assert p0 > 85000 and expected > 40
    assert abs((p0 - p1) - expected) <= 1.0, (p0, p1, expected)


# ---- the conditions that make the GPU tests non-vacuous, on the oracle alone, for exactly their inputs ------------------------------------
def _conditions(x, twin, ppm, invert=None, name=""):
    Cn = x.shape[0]
    inv = np.zeros(Cn, dtype=np.uint8) if invert is None else invert
    rows, _, logs = oc.oracle_of("cond " + name, x, inv, logs=True)
    trows, _, _ = oc.oracle_of("cond twin " + name, twin, inv)
    moves = [oc.index_moves(lg) for lg in logs]
    for c in range(Cn):
        if 200 <= abs(ppm[c]) <= 800:
            assert trows[c].size >= 30, (c, trows[c].size)
            assert rows[c].size >= 0.9 * trows[c].size, (c, ppm[c], rows[c].size, trows[c].size)
            assert moves[c] >= 10, (c, ppm[c], moves[c])
    fast = [c for c in range(Cn) if abs(ppm[c]) >= 1000]
    assert any(oc.lost_and_regained(logs[c]) for c in fast)
    return moves


def test_the_main_batch_moves_the_clock_and_still_decodes():
    b = oc.main()
    assert b["x"].shape == (oc.MAIN_C, oc.MAIN_T)
    for v in oc.PPM_GRID:                                   # each value of the grid on several channels
        assert (b["ppm"] == v).sum() >= 4, v
    assert set(b["kind"].tolist()) == {0, 1, 2, 4} and set(b["sigma"].tolist()) == {0.0, 300.0, 1200.0}
    moves = _conditions(b["x"], b["twin"](), b["ppm"], name="main")
    # the measured counts (NOTES.md): about one move per 10 / (|ppm| * 1e-6) samples while a transmission is locked
    for lo, hi, v in ((15, 30, 200), (40, 55, 500), (40, 80, 800)):
        got = [moves[c] for c in range(oc.MAIN_C) if abs(b["ppm"][c]) == v]
        assert min(got) >= lo and max(got) <= hi, (v, got)
    on_clock = [moves[c] for c in range(oc.MAIN_C) if b["ppm"][c] == 0]
    assert max(on_clock) < 20                               # (what the suite had before: hardly any)


def test_the_mixed_polarity_batch_moves_the_clock_and_still_decodes():
    x, pol = oc.main_mixed_polarity()
    b = oc.main()
    assert 16 < int(pol.sum()) < 48
    twin = np.where(pol[:, None] == 1, oc.negated(b["twin"]()), b["twin"]())
    _conditions(x, twin, b["ppm"], invert=pol, name="mixed")
    # the polarity decides what a channel reports: under the wrong one an inverted channel does not yield its frames
    rows, _, _ = oc.oracle_of("cond mixed", x, pol, logs=True)
    wrong, _, _ = oc.oracle_of("cond mixed wrong", x, pol ^ 1)
    for c in np.flatnonzero(pol):
        if 200 <= abs(b["ppm"][c]) <= 800:
            assert wrong[c].size < rows[c].size, c


def test_the_reset_case_restarts_inside_drifting_transmissions():
    """tests/test_gpu_off_clock.py resets RESET_CHANNELS in front of the second run of 48 000 samples: on the oracle, a fresh demodulator started
    there finds the transmission again on most of them, and reports something else than the continued one."""
    x = oc.main()["x"]
    half = oc.MAIN_T // 2
    rows, _, _ = oc.oracle_of("cond main", x, None, logs=True)
    fresh, _, lg = oc.oracle_of("reset fresh", x[oc.RESET_CHANNELS, half:], None, logs=True)
    found = 0
    for i, c in enumerate(oc.RESET_CHANNELS):
        going = rows[c][rows[c]["sample_pos"] >= half]
        assert fresh[i].tobytes() != going.tobytes(), c
        found += int(fresh[i].size >= 10)
    assert 2 * found >= len(oc.RESET_CHANNELS), found
    ppm = oc.main()["ppm"][list(oc.RESET_CHANNELS)]
    assert sum(1 for v in ppm if 200 <= abs(v) <= 800) >= 4 and len({abs(v) for v in ppm}) >= 6
    assert sum(oc.index_moves(l) for l in lg) > 100


def test_the_bursty_batch_drifts_and_closes_the_gate():
    x, _ = oc.bursty()
    rows, diags, logs = oc.oracle_of("bursty", x, None, logs=True)
    assert sum(r.size for r in rows) > 8 * x.shape[0]
    # at 500 ppm sample_index moves once per 2000 samples locked, about once per frame: a channel that reports ten frames shows five moves at least
    for c in range(x.shape[0]):
        if rows[c].size >= 10:
            assert oc.index_moves(logs[c]) >= 5, (c, rows[c].size, oc.index_moves(logs[c]))
    assert sum(1 for r in rows if r.size >= 10) >= x.shape[0] // 2
    assert sum(1 for lg in logs if (np.diff(lg["dcd"].astype(np.int32)) < 0).any()) >= x.shape[0] // 2   # the carrier detect does go off


@pytest.mark.parametrize("seed", oc.SCENARIO_SEEDS)
def test_the_resampled_random_scenarios_decode_and_drift(seed):
    x, ppm = oc.scenarios(seed, 32)
    assert len(set(np.abs(ppm).tolist())) >= 5
    rows, _, logs = oc.oracle_of(("scenarios", seed), x, None, logs=True)
    assert sum(r.size for r in rows) > 4 * x.shape[0]
    # (bursts of a few frames with a random symbol phase each: sample_index moves with every acquisition here, on the clock as well; what these
    #  inputs add is the drift on top of lost syncs, forced unlocks and filter restarts, not a count of their own)
    assert sum(oc.index_moves(lg) for lg in logs) > 4 * x.shape[0]
    n = x.shape[1] + 256
    for c in range(x.shape[0]):
        assert (ppm[c] == 0) == np.array_equal(x[c], ol.random_scenario(seed * 1000 + c, total=n)[: x.shape[1]]), c


def test_the_kalman_orders_differ_in_the_clock_estimate_at_500_ppm():
    """tests/test_gpu_off_clock.py runs the first 32 channels x 48 000 samples of the main batch under every evaluation order of the 2 x 2
    Kalman arithmetic: on the oracle, at +-500 ppm, two orders end with different `clock` words on some channel — off the clock the second
    state is 5e-4, not 1e-7, and its last place shows the order."""
    b = oc.main()
    chs = [c for c in range(32) if abs(b["ppm"][c]) == 500]
    assert len(chs) >= 4
    x = np.ascontiguousarray(b["x"][chs, :48000])
    lib = ol.oracle()
    words = {}
    try:
        for order in oc.KALMAN_ORDERS:
            lib.m17o_set_kalman_order(C.c_int(order))
            _, _, d = ol.demod_batch(x, cap=64, threads=oc.THREADS)
            words[order] = d["clock"].view(np.uint32).copy()
            assert (np.abs(np.abs(d["clock"]) - 5e-4) < 1e-4).any(), d["clock"]
    finally:
        lib.m17o_set_kalman_order(C.c_int(3))
    assert any((words[a] != words[b_]).any() for a in words for b_ in words if a < b_), words


# ---- the oracle against the reference composition, off the clock ---------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(os.path.join(ol.ORACLE_DIR, "_ref", "libm17ref.so")), reason="oracle/_ref not built (reference not present)")
def test_the_orchestrator_over_the_references_own_operators_equals_the_oracle_off_clock():
    """tests/test_oracle_vs_ref.py's composition check on 28 random scenarios re-read at +-60 .. +-2000 ppm, either polarity: records, the last
    diagnostic callback and every diagnostic callback in order, byte for byte."""
    grid = [v for v in oc.PPM_GRID if abs(v) >= 60]
    frames = moves = 0
    for seed in range(28):
        ppm = grid[seed % len(grid)]
        x = oc.resample_clock(ol.random_scenario(5000 + seed, total=96000 + 256), ppm)[:96000]
        inv = seed & 1
        ro, do = ol.demod(x, invert=inv)
        rh, dh = ol.hybrid_demod(x, invert=inv)
        assert ro.tobytes() == rh.tobytes(), (seed, ppm)
        assert do.tobytes() == dh.tobytes(), (seed, ppm)
        lo = ol.demod_diag_log(x, invert=inv)
        assert lo.tobytes() == ol.hybrid_diag_log(x, invert=inv).tobytes(), (seed, ppm)
        frames += ro.size
        moves += oc.index_moves(lo)
    assert frames > 300 and moves > 100, (frames, moves)
