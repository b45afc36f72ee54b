"""CPU: the REFERENCE's own demodulator (M17Demodulator.h, ClockRecovery.h, FreqDevEstimator.h, KalmanFilter.h compiled as they lie over the blaze
stand-in of oracle/blaze_min, one build per evaluation order) against the oracle's restatement of it, m17_oracle_demod.hpp, under the same order: every
frame callback and every diagnostic callback, in order, every float bit for bit.  tests/ref_demod_lib.py has the input set and the plumbing.

The live tests are skipped where oracle/_ref is absent, as tests/test_oracle_vs_ref.py is; the frozen copy (tests/golden/ref_demod_vectors.npz) is
compared with the oracle everywhere."""
import numpy as np
import pytest

import boundary_phases as bp
import off_clock as oc
import ref_demod_lib as rl

live = pytest.mark.skipif(not rl.have_ref(), reason="oracle/_ref not built (reference not present)")

_CACHE = {}
COUNTS = {}                 # (family, order) -> (channels, frame callbacks, diagnostic callbacks), for whoever wants the table of NOTES.md again


def _rows(family):
    if family not in _CACHE:
        _CACHE[family] = rl.family_rows(family)
    return _CACHE[family]


def _compare(family, order, rows, inverts, names):
    ref = rl.ref_demod_many(rows, inverts, order)
    ora = rl.oracle_demod_many(rows, inverts, order)
    for i, name in enumerate(names):
        d = rl.first_difference(ref[i], rl.masked(ora[i]))
        assert d is None, f"{family} {name} order {order}: reference against oracle: {d}"
    COUNTS[(family, order)] = (len(rows), sum(r[0].size for r in ref), sum(r[1].size for r in ref))
    return ref, ora


@live
@pytest.mark.parametrize("order", [0, 3])
@pytest.mark.parametrize("family", list(rl.FAMILIES))
def test_the_references_demodulator_equals_the_oracle(family, order):
    """Orders 0 (eager) and 3 (the default) over the whole input set."""
    rows, inverts = _rows(family)
    ref, ora = _compare(family, order, rows, inverts, rl.FAMILIES[family])
    if family == "random":
        frames = np.concatenate([r[0] for r in ref])
        assert frames.size > 2500 and int(np.bitwise_or.reduce(1 << frames["frame_type"].astype(np.int64))) == 0b101111   # (as the hybrid test finds them)
    if family == "silent":              # DataCarrierDetect's 0 / 0: both agree that nothing is ever decoded, and the oracle's level is NaN
        assert ref[0][0].size == 0 and ora[0][0].size == 0 and ref[0][1].size > 50 and np.isnan(ora[0][1]["dcd_level"][-1])
        assert not ref[0][1]["dcd"].any() and not ref[0][1]["locked"].any()


@live
@pytest.mark.parametrize("order", [1, 2, 4, 5, 6, 7])
def test_the_other_orders_on_random_scenarios(order):
    rows, inverts = _rows("random")
    n = len(rl.OTHER_ORDER_SEEDS)
    _compare("random", order, rows[:n], inverts[:n], rl.OTHER_ORDER_SEEDS)


@live
def test_the_comparison_tells_the_orders_apart():
    """The reference built for order 0 against the oracle under order 3, and the other way round: the low bits of offset and deviation differ on most
    scenarios (measured: 20 of 24 either way), so an order that did not correspond would show."""
    rows, inverts = _rows("random")
    n = len(rl.OTHER_ORDER_SEEDS)
    for a, b in ((0, 3), (3, 0)):
        ref = rl.ref_demod_many(rows[:n], inverts[:n], a)
        ora = rl.oracle_demod_many(rows[:n], inverts[:n], b)
        differ = sum(rl.first_difference(ref[i], rl.masked(ora[i])) is not None for i in range(n))
        assert differ >= n // 3, (a, b, differ)


# ---- what the rare-branch families are in the set for, asserted on the subsets taken ------------------------------------------------------------
def _oracle_subset(family):
    key = ("oracle", family)
    if key not in _CACHE:
        rows, inverts = _rows(family)
        _CACHE[key] = rl.oracle_demod_many(rows, inverts, 3)
    return _CACHE[key]


@pytest.mark.parametrize("name", bp.BATCHES)
def test_the_boundary_phase_subsets_still_show_forced_unlocks(name):
    """tests/test_boundary_phases.py test_forced_unlocks_at_many_phases, on every 7th channel: more than half of the subset's channels show `locked` falling
    with the carrier still there (the whole batches: 1863, 1771 and 1328 of 1920), and the carrier detect changes on every channel."""
    ora = _oracle_subset("bp_" + name)
    forced = changed = 0
    for recs, log in ora:
        pos = oc.log_pos(log).astype(np.int64)
        forced += bool(bp.forced_unlocks_of(log, pos, np.zeros(log.size, dtype=np.int64))[0].size)
        changed += bool((log["dcd"][1:] != log["dcd"][:-1]).any())
    assert 2 * forced > len(ora) and changed == len(ora), (name, forced, changed, len(ora))


def _gave_up(c, pair):
    return bp.gave_up_packet_sync(pair[0], pair[1], (bp.hole_span(c)[0], bp.T))


def test_the_hole_batch_reaches_the_give_up_branch_of_packet_sync():
    """tests/test_boundary_phases.py test_packet_hole_reaches_the_give_up_branch_of_packet_sync: the whole batch is in the set, at least 100 of its 384
    channels give up in do_packet_sync — and so do the hole channels of the frozen copy."""
    ora = _oracle_subset("bp_hole")
    gave = [c for c, pair in zip(rl.FAMILIES["bp_hole"], ora) if _gave_up(c, pair) is not None]
    assert len(gave) >= 100, len(gave)
    frozen = [i for f, i in rl.FIXTURE_CHANNELS if f == "bp_hole"]
    assert len(frozen) >= 4 and set(frozen) <= set(gave), sorted(set(frozen) - set(gave))


def test_the_off_clock_rows_move_the_sample_index():
    """tests/test_off_clock.py's condition on the rows taken: clock_recovery.update() moves sample_index inside running transmissions."""
    ora = _oracle_subset("oc_main")
    assert sum(oc.locked_moves(log) for _, log in ora) > 300
    frozen = [i for f, i in rl.FIXTURE_CHANNELS if f == "oc_main"]
    assert sum(oc.locked_moves(ora[i][1]) for i in frozen) >= 40


# ---- clock recovery and deviation estimator, value for value -----------------------------------------------------------------------------------
def _check_clock_premises(order, seqs, traces):
    """The cases the sequences are there for, read off the traces themselves."""
    below = above = down = up = neg = half = 0
    dts = set()
    for seq, tr in zip(seqs, traces):
        for z0, st, z, dt in rl.kalman_calls(seq):
            dts |= set(dt.tolist())
            x0, x1 = np.float32(z0), np.float32(0)
            for k, s in enumerate(st):
                prior = np.float32(x0 + np.float32(np.float32(dt[k]) * x1))     # F x: 1 * x0 + dt * x1, in float
                d = float(np.float32(z[k] - prior))
                below += -5.5 < d < -5.0
                above += 5.0 < d < 5.5
                zz = z[k] + 10 if d < -5.0 else z[k] - 10 if d > 5.0 else z[k]
                x0, x1 = np.float32(tr[s, 3]), np.float32(tr[s, 4])
                down += zz > prior and x0 < prior - 5        # carried to 10 or above, brought back
                up += zz < prior and x0 > prior + 5          # carried below 0, brought back
        for _, a in rl.free_run_arguments(seq, tr):
            neg += a < 0
            half += (abs(a) % 1.0) == 0.5
    assert below and above and down and up, (order, below, above, down, up)
    assert {0, 1, 1920, 19200} <= dts
    assert neg and half, (order, neg, half)


@live
@pytest.mark.parametrize("order", rl.ORDERS)
def test_clock_recovery_values(order):
    """ClockRecovery<float,10> of the reference against the oracle's: sample_index and clock_estimate after every step, and the filter's x and P after every
    update(index), over reset / count / update(index) / update() sequences that hold the wrap cases, dt = 0, 1, 1920 and 19 200, a negative fmod
    argument and an exact x.5."""
    seqs = rl.clock_sequences()
    traces = [rl.ref_clock_trace(order, s) for s in seqs]
    _check_clock_premises(order, seqs, traces)
    with rl.oracle_order(order):
        for j, (seq, tr) in enumerate(zip(seqs, traces)):
            si, ce, kal = rl.oracle_clock_trace(seq)
            assert np.array_equal(tr[:, 0], si.astype(np.float32)), (order, j)
            assert rl.same_bits(np.ascontiguousarray(tr[:, 1]), ce), (order, j)
            for st, o in kal:
                assert rl.same_bits(np.ascontiguousarray(tr[st, 3:9]), o), (order, j)
                assert rl.same_bits(np.ascontiguousarray(tr[st, 2]), np.ascontiguousarray(o[:, 0])), (order, j)      # sample_estimate_ is x0


@live
@pytest.mark.parametrize("order", rl.ORDERS)
def test_deviation_estimator_values(order):
    """FreqDevEstimator<float>::update of the reference against the oracle's: idev, offset and deviation after every update, NaN and infinity included."""
    rows = rl.dev_sequences()
    traces = [rl.ref_dev_trace(order, r) for r in rows]
    assert traces[0].shape[0] == 2000 and np.isfinite(traces[0]).all()
    assert np.isinf(traces[1][[0, 20], 0]).all() and np.isfinite(traces[1][[19, 39, 59], 0]).all()              # mn == mx
    assert np.isnan(traces[2][10, 1]) and np.isfinite(traces[2][11:30]).all() and np.isfinite(traces[2][47:]).all()   # NaN, and back through reset_
    with rl.oracle_order(order):
        for j, (r, tr) in enumerate(zip(rows, traces)):
            assert rl.same_bits(tr, rl.oracle_dev_trace(r)), (order, j)


# ---- the frozen copy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
def test_the_oracle_equals_the_recorded_reference(order):
    """Everywhere, the reference present or not: the oracle over the regenerated fixture rows (hashes checked: a different row FAILS) equals what the
    reference's demodulator was recorded to deliver, callback for callback."""
    z = rl.load_fixture()
    x, pol = rl.fixture_rows()
    ora = rl.oracle_demod_many(list(x), pol.tolist(), order)
    frames = 0
    for i, name in enumerate(rl.FIXTURE_CHANNELS):
        exp = rl.fixture_channel(z, order, i)
        d = rl.first_difference(exp, rl.masked(ora[i]))
        assert d is None, f"{name} order {order}: recorded reference against oracle: {d}"
        assert np.array_equal(z[f"last_diag_o{order}"].view(rl.ol.DIAG).reshape(-1)[i:i + 1].tobytes(), exp[1][-1:].tobytes())
        frames += exp[0].size
    assert frames > 10 * len(rl.FIXTURE_CHANNELS)


@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
def test_the_oracle_equals_the_recorded_clock_and_deviation_traces(order):
    z = rl.load_fixture()
    seqs, rows = rl.clock_sequences(), rl.dev_sequences()
    traces = [z[f"clock_o{order}_{j}"] for j in range(len(seqs))]
    _check_clock_premises(order, seqs, traces)
    with rl.oracle_order(order):
        for j, (seq, tr) in enumerate(zip(seqs, traces)):
            si, ce, kal = rl.oracle_clock_trace(seq)
            assert np.array_equal(tr[:, 0], si.astype(np.float32)) and rl.same_bits(np.ascontiguousarray(tr[:, 1]), ce), (order, j)
            for st, o in kal:
                assert rl.same_bits(np.ascontiguousarray(tr[st, 3:9]), o), (order, j)
        for j, r in enumerate(rows):
            assert rl.same_bits(z[f"dev_o{order}_{j}"], rl.oracle_dev_trace(r)), (order, j)


@live
@pytest.mark.parametrize("order", rl.FIXTURE_ORDERS)
def test_the_recorded_reference_is_what_the_reference_delivers_now(order):
    """Where the reference is present: the file is not stale."""
    z = rl.load_fixture()
    x, pol = rl.fixture_rows()
    ref = rl.ref_demod_many(list(x), pol.tolist(), order)
    for i, name in enumerate(rl.FIXTURE_CHANNELS):
        assert rl.first_difference(ref[i], rl.fixture_channel(z, order, i)) is None, name
    for j, s in enumerate(rl.clock_sequences()):
        assert rl.same_bits(rl.ref_clock_trace(order, s), z[f"clock_o{order}_{j}"])
    for j, r in enumerate(rl.dev_sequences()):
        assert rl.same_bits(rl.ref_dev_trace(order, r), z[f"dev_o{order}_{j}"])
