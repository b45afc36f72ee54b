"""GPU tests of runs longer than 10 s, up to M17HIP_MAX_SAMPLES_PER_RUN (include/m17hip.h: 33 553 152 samples per channel, 11.6 minutes,
700 segments): the HIP path, called through the C ABI, against the CPU oracle on identical seeded inputs, in the shape of
tests/test_gpu_parity.py — records and integer diagnostics byte for byte, float outputs bit for bit, no tolerance anywhere.

What only runs, or only runs this way, beyond 10 s: the second and later 512-slot passes of decode_deferred_kernel and deferred-cost tags
with slot numbers above 511; buffer descriptors and 32-bit byte offsets sized from T (sixteen channel rows of the limit-filter replay end
less than 16 KB below the offset that stands for "no store"); hundreds of segments queued ahead (event vectors, forecasts, two-parity EVM
cursors); the K3 table, the record stride, the deferred-LLR store, the compaction and the synthesis symbol buffer at tens of thousands of
frames per channel.

Every test first asserts ON THE ORACLE'S OUTPUT ALONE that its input reaches what it is meant to reach (a generator change cannot quietly
turn it into a short-run test), and every channel of a batch is compared.  Positions are subsampled in one place only: the K3 table of the
per-operator test (two sums per start tick: a full recomputation is quadratic)."""
import concurrent.futures
import ctypes as C
import os
import re

import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = int(re.search(r"#define M17HIP_MAX_SAMPLES_PER_RUN (\d+)u", open(os.path.join(ROOT, "include", "m17hip.h")).read()).group(1))
THREADS = 16
EINVAL = -1
INT_FIELDS = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "pad")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock", "dcd_level")
DEFERRED_TYPES = (2, 5)      # stream / BERT payload frames: the records whose decoding the sequential kernel hands over


def _par(fn, items):
    """fn over items on a thread pool (the oracle's entry points are foreign calls: the interpreter lock is released)."""
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(fn, items))


def _oracle(x, invert=0):
    """Per-channel record arrays and the m17_diag block of every channel."""
    T = x.shape[1]
    recs, counts, diags = ol.demod_batch(x, invert=invert, cap=2 * (T // 1920 + 2) + 4, threads=THREADS)
    return [recs[c, : counts[c]].copy() for c in range(x.shape[0])], diags


def _rows64(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, 64)


def _assert_records(got, per, what, T=0):
    """got == the oracle's records of EVERY channel, byte for byte; a failure names channels, seq, slot and position (is the slot beyond the
    first 512-slot pass, is the sample beyond a 2^31-byte offset of a [channels][T] float slab)."""
    exp = np.concatenate(per)
    if got.tobytes() == exp.tobytes():
        return
    lines = [f"{what}: records differ, {got.size} fetched / {exp.size} expected"]
    for c, e in enumerate(per):
        g = got[got["channel"] == c]
        n = min(g.size, e.size)
        bad = np.flatnonzero((_rows64(g[:n]) != _rows64(e[:n])).any(axis=1))
        if g.size == e.size and bad.size == 0:
            continue
        line = f"channel {c}: {g.size}/{e.size} records, {bad.size} differ"
        if bad.size:
            i = int(bad[0])
            fields = [f for f in e.dtype.names if not np.array_equal(g[i][f], e[i][f])]
            line += (f"; first at slot {i} (seq {int(e[i]['seq'])}, slot >= 512: {i >= 512}, sample_pos {int(e[i]['sample_pos'])}, byte offset in a [C][T] float slab >= 2^31: "
                     f"{4 * (c * T + int(e[i]['sample_pos'])) >= 1 << 31}, type {int(e[i]['frame_type'])}) in {fields}; last at slot {int(bad[-1])}")
        lines.append(line)
        if len(lines) > 12:
            break
    raise AssertionError("\n".join(lines))


def _assert_diag(d, diags, what):
    for f in INT_FIELDS:
        assert np.array_equal(d[f], diags[f]), (what, f, np.flatnonzero((d[f] != diags[f]).reshape(len(d), -1).any(axis=1))[:16].tolist())
    for f in FLOAT_FIELDS:
        assert np.array_equal(d[f], diags[f], equal_nan=True), (what, f)


def _assert_row_equal(got, exp, what):
    """One float row bit for bit, as the rest of the suite compares (np.array_equal); a failure names the first and last differing sample."""
    if np.array_equal(got, exp):
        return
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.size} of {exp.size} values differ, first at {i} (byte offset {4 * i:#x}: got {got[i]!r}, expected {exp[i]!r}), "
                         f"last at {int(bad[-1])}")


def _run_and_check(x, per, diags, tune=None, flags=0, what=""):
    """One context of exactly the input's size: upload, run, records and m17_diag against the oracle's; the context is closed."""
    Cn, T = x.shape
    ctx = m17hip.Context(Cn, T)
    try:
        for k, v in (tune or {}).items():
            ctx.tune(k, v)
        ctx.upload(x)
        ctx.reset()
        ctx.run(flags=flags)
        got = ctx.frames()
        d = ctx.diag(Cn)
        drops = ctx.replay_drops()
    finally:
        ctx.close()
    _assert_records(got, per, what, T)
    _assert_diag(d, diags, what)
    return drops


# ------------------------------------------------------------------------------------------------ 1: across the 512-slot passes --
CASE1_SIGMA = (600.0, 600.0, 300.0, 900.0)
CASE1_OFFSETS = (None, None, 6, 5, 3, 3, 2, 2, 1, 1, 0, 0, -1, -1, -2, -2, -3, -3, -5, -6, None, None, None, None)   # None: lead-in 3072
CASE1_BURSTS = {20: 300000, 21: 320000, 22: 340000, 23: 360000}   # these channels: transmissions of this many samples, the last 30 frames of each loud noise


def _case1_input(T, near):
    """24 channels, even BERT / odd voice, whose lead-ins (loud noise before the transmission) put the number of records a channel ends with
    a few below, at and a few above `near`; four channels are one transmission after the other with noise loud enough in between to lose sync
    (the forced unlock) and acquire the next one."""
    rows = []
    for c, off in enumerate(CASE1_OFFSETS):
        if c in CASE1_BURSTS:
            n = CASE1_BURSTS[c]
            parts = [ol.generate_batch(ol.gen_params(seed=4200 + k, kind=-1, n_frames=n // 1920 - 30, lead_in=3072, noise_sigma=600.0, tail_sigma=3000.0,
                                                     lead_sigma=40000.0, total=n), 1, n, threads=1, chan0=c)[0] for k in range(T // n + 1)]
            rows.append(np.concatenate(parts)[:T])
            continue
        lead = 3072 if off is None else T - 1920 * (near + 3 + off)
        sigma = CASE1_SIGMA[c % 4]
        p = ol.gen_params(seed=4107, kind=-1, n_frames=T // 1920, lead_in=lead, noise_sigma=sigma, tail_sigma=sigma, lead_sigma=40000.0, total=T)
        rows.append(ol.generate_batch(p, 1, T, threads=1, chan0=c)[0])
    return np.stack(rows)


def _case1(T, near):
    """Input and oracle output of case 1, with what the case is meant to reach asserted on the oracle's output alone."""
    x = _case1_input(T, near)
    per, diags = _oracle(x)
    counts = np.array([p.size for p in per])
    assert (counts > 512).sum() >= len(per) // 4, counts.tolist()
    if near == 1024:
        assert (counts > 1024).sum() >= 2, counts.tolist()
    assert ((counts >= near - 8) & (counts < near)).any() and ((counts > near) & (counts <= near + 8)).any(), counts.tolist()   # just below, just above
    seqs = np.concatenate([p["seq"][np.isin(p["frame_type"], DEFERRED_TYPES)] for p in per])
    assert ((seqs >= near - 2) & (seqs <= near + 2)).any()
    regained = 0
    for p in per:       # a gap of more than four frames between two records, and at least ten records behind it: sync was lost and found again
        gaps = np.flatnonzero(np.diff(p["sample_pos"].astype(np.int64)) > 4 * 1920)
        regained += int(gaps.size > 0 and p.size - 1 - int(gaps[0]) >= 10)
    assert regained >= 2, regained
    return x, per, diags


@pytest.fixture(scope="module", params=[(1100000, 512), (2100000, 1024)], ids=["1.1M", "2.1M"])
def passes(request):
    return _case1(*request.param)


@pytest.mark.parametrize("tune", [{}, {15: 0, 17: 0}, {20: 1}], ids=["default", "decode_and_evm_in_k5", "redo_in_front"])
def test_across_the_passes_of_the_deferred_decode(passes, tune):
    """decode_deferred_kernel works through a channel's records 512 slots at a time: runs of 1.1 M and 2.1 M samples end with channels a few
    records below 512 / 1024, at them and a few above (two and three passes, the last one of a handful of slots), tags DEFER_TAG | slot with
    slots above 511 are produced and resolved — with the default knobs, with every frame decoded and the EVM folded in the sequential kernel
    (keys 15, 17 = 0: what the deferred forms must equal), and with the replay's redo in front of it (key 20 = 1)."""
    x, per, diags = passes
    _run_and_check(x, per, diags, tune=tune, what=f"T={x.shape[1]} {tune}")


# ------------------------------------------------------------------------------------------------ 2, 3: at the limit --------------
class _Limit:
    pass


def _limit_batch():
    """17 channels of L samples (even BERT, odd voice): row 15 of a full sixteen-row replay group and a partial group; the oracle's records."""
    b = _Limit()
    b.params = ol.gen_params(seed=20261016, kind=-1, n_frames=L // 1920 - 6, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0, total=L)
    b.x = ol.generate_batch(b.params, 17, L, threads=THREADS)
    b.per, b.diags = _oracle(b.x)
    _assert_reaches_the_end(b.per, L)
    return b


@pytest.fixture(scope="module")
def limit():
    return _limit_batch()


def _assert_reaches_the_end(per, T):
    for c, p in enumerate(per):
        assert p.size > 17000 and int(p["sample_pos"].max()) > T - 4000, (c, p.size, int(p["sample_pos"].max()) if p.size else None)


def test_ctx_create_refuses_one_sample_beyond_the_limit():
    lib = m17hip.load_library()
    h = C.c_void_p()
    assert lib.m17hip_ctx_create(0, C.c_uint32(1), C.c_uint32(L + 1), C.byref(h)) == EINVAL and not h.value


def test_at_the_limit(limit):
    """T = M17HIP_MAX_SAMPLES_PER_RUN, 17 channels, default segmenting: 700 segments queued ahead, sixteen rows of ypitch floats ending
    below the replay's "no store" offset, 17 460 records per channel."""
    _run_and_check(limit.x, limit.per, limit.diags, what="T=L")


@pytest.mark.parametrize("short", [1, 127])
def test_just_below_the_limit(limit, short):
    """T = L - 1 and L - 127: not a multiple of 8 / 128 / 192 / 1920, in a context of exactly that size."""
    T = L - short
    x = np.ascontiguousarray(limit.x[14:17, :T])
    per, diags = _oracle(x)
    _assert_reaches_the_end(per, T)
    _run_and_check(x, per, diags, what=f"T=L-{short}")


def test_one_segment_at_the_limit(limit):
    """m17hip_tune key 3 = 0: the whole run is one K2 + K5 launch over 33.5 M samples.  All 17 channels: a segment's rows are addressed from
    the segment's first sample, so it is HERE, and not with the default segmenting, that row 15 of the replay's sixteen-row descriptor ends
    a few KB below the offset that stands for "no store" (with the descriptor's size clamp lowered by 1 MB this test fails, the segmented
    one does not)."""
    _run_and_check(limit.x, limit.per, limit.diags, tune={3: 0}, what="T=L, one segment")


# ------------------------------------------------------------------------------------------------ 4: late events -----------------
def _bursty(Cn, T, seed):
    """Short transmissions of every kind between stretches of loud, quiet and no noise (as test_gate_aware_front_end_on_bursty_channels makes
    them); every fourth channel is generated with inverted polarity.  Returns the input and, per channel, where each transmission starts."""
    rng = np.random.default_rng(seed)
    x = np.zeros((Cn, T), dtype=np.int16)
    starts = []
    for c in range(Cn):
        pos, st = 0, []
        while pos < T - 9000:
            n = min(int(rng.integers(9000, 70000)), T - pos)
            p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.choice([0, 1, 2, 4])), n_frames=int(rng.integers(1, 9)),
                              lead_in=int(rng.integers(0, 6000)), lead_sigma=float(rng.choice([100.0, 20000.0, 40000.0])),
                              noise_sigma=float(rng.choice([100.0, 600.0, 1500.0])), tail_sigma=float(rng.choice([100.0, 5000.0, 20000.0])),
                              phase=int(rng.integers(-1, 10)), invert=int(c % 4 == 3), total=n)
            x[c, pos:pos + n] = ol.generate(p)[:n]
            st.append(pos)
            pos += n
        x[c, pos:] = rng.integers(-300, 300, T - pos)
        starts.append(np.array(st + [T], dtype=np.int64))
    return x, starts


def _late_frames(per, starts, T):
    """Per channel: the records that belong to transmissions which START in the last third of the run."""
    out = []
    for p, st in zip(per, starts):
        pos = p["sample_pos"].astype(np.int64)
        begin = st[np.searchsorted(st, pos, side="right") - 1]      # start of the transmission the record's sample lies in
        out.append(int((begin >= 2 * T // 3).sum()))
    return np.array(out)


def _late_case():
    """Input and oracle output (both polarities) of case 4; asserted on the oracle's records: every channel of the polarity that decodes
    holds frames of transmissions that start in the last third of the run."""
    Cn, T = 16, 5000000
    x, starts = _bursty(Cn, T, seed=5150)
    normal = [c for c in range(Cn) if c % 4 != 3]
    inverted = [c for c in range(Cn) if c % 4 == 3]
    oracle = {0: _oracle(x), 1: _oracle(x, invert=1)}
    for inv, decoding in ((0, normal), (1, inverted)):
        late = _late_frames(oracle[inv][0], starts, T)
        assert (late[decoding] > 0).all() and int(late[decoding].sum()) > 20 * len(decoding), (inv, late.tolist())
    return x, oracle


def test_late_events_far_beyond_the_tenth_segment():
    """5 M samples (105 segments) of many short transmissions: forced unlocks, replay drops, redos and re-acquisitions in segment k >> 10,
    the gate-aware forecast (key 26) on and off, a ramp of first segments (key 33 = 9600), and the other polarity (M17HIP_FLAG_INVERT)."""
    x, oracle = _late_case()
    for tune, flags in (({26: 1}, 0), ({26: 0}, 0), ({33: 9600}, 0), ({}, m17hip.FLAG_INVERT)):
        per, diags = oracle[flags]
        drops = _run_and_check(x, per, diags, tune=tune, flags=flags, what=f"late events {tune} flags={flags}")
        assert drops > 0, (tune, flags)


# ------------------------------------------------------------------------------------------------ 5: a continued stream ----------
def _stream_case():
    """Input, oracle output and run lengths of case 5; asserted on the oracle's records: every run of every channel holds more than 512."""
    Cn, lengths = 16, [1100000, 1234567, 1100000]
    T = sum(lengths)
    p = ol.gen_params(seed=5501, kind=-1, n_frames=T // 1920, lead_in=3072, noise_sigma=700.0, tail_sigma=700.0, lead_sigma=40000.0, total=T)
    x = ol.generate_batch(p, Cn, T, threads=THREADS)
    per, diags = _oracle(x)
    cuts = np.cumsum([0] + lengths)
    for c, r in enumerate(per):      # every run of every channel goes beyond the first 512-slot pass
        in_run = np.histogram(r["sample_pos"].astype(np.int64), bins=cuts)[0]
        assert (in_run > 512).all(), (c, in_run.tolist())
    return x, per, diags, lengths, cuts


def test_a_continued_stream_of_long_runs():
    """Three runs of 1.1-1.2 M samples fed as a live feed does (tests/test_gpu_streaming.py): run k + 1 staged, its front end and its run queued,
    THEN run k's records fetched (m17hip_frames_select(ctx, 1)) — both record sets and both deferred-frame stores hold more than 512 records
    per channel, and the deferred decode of run k works beside run k + 1.  The union of the fetched records == the oracle's demodulation of
    the concatenated input."""
    import torch
    x, per, diags, lengths, cuts = _stream_case()
    Cn = x.shape[0]
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, a:b])).pin_memory() for a, b in zip(cuts[:-1], cuts[1:])]
    ctx = m17hip.Context(Cn, max(lengths))
    try:
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), Cn, lengths[0])
        ctx.run(channels=Cn, samples=lengths[0])
        parts = []
        for k in range(len(lengths)):
            if k + 1 < len(lengths):
                ctx.upload_async(pins[k + 1].data_ptr(), Cn, lengths[k + 1])
                ctx.front(channels=Cn, samples=lengths[k + 1])
                ctx.run(channels=Cn, samples=lengths[k + 1])
                ctx.frames_select(1)
            parts.append(ctx.frames().copy())
            ctx.frames_select(0)
        ctx.upload_wait()
        d = ctx.diag(Cn)
    finally:
        ctx.close()
    for k, part in enumerate(parts):   # run k's fetch delivered run k's records and nothing else
        pos = part["sample_pos"].astype(np.int64)
        assert part.size > 512 * Cn and (pos >= cuts[k]).all() and (pos < cuts[k + 1]).all(), k
    got = np.concatenate(parts)
    _assert_records(got[np.lexsort((got["seq"], got["channel"]))], per, "continued stream")
    _assert_diag(d, diags, "continued stream")


# ------------------------------------------------------------------------------------------------ 6: consumers and logs ----------
def _consumers_case():
    """Input and oracle output of case 6 (records, m17_diag, every diagnostic callback, the PRBS9 receiver's counts); asserted on them: half of
    the channels beyond 1024 records, thousands of callbacks per channel, thousands of BERT frames and some bit errors."""
    Cn, T = 12, 2100000
    sigmas = (300.0, 600.0, 2600.0, 1500.0, 3400.0, 2600.0)
    rows = []
    for c in range(Cn):
        p = ol.gen_params(seed=6601, kind=-1, n_frames=T // 1920, lead_in=3072, noise_sigma=sigmas[c % 6], tail_sigma=500.0, lead_sigma=40000.0, total=T)
        rows.append(ol.generate_batch(p, 1, T, threads=1, chan0=c)[0])
    x = np.stack(rows)
    per, diags = _oracle(x)
    room = T // 384 + 2
    logs = _par(lambda c: ol.demod_diag_log(x[c], cap=room), range(Cn))
    stats = [ol.bert_count(r[r["frame_type"] == 5]["payload"][:, :25]) if (r["frame_type"] == 5).any() else (0, 0, False) for r in per]
    assert sum(r.size > 1024 for r in per) >= Cn // 2 and min(lg.size for lg in logs) > 2048
    assert sum(s[1] for s in stats) > 0 and sum(int((r["frame_type"] == 5).sum()) for r in per) > 2048
    return x, per, diags, logs, stats, room


def test_consumers_and_the_diagnostic_log_over_a_long_run():
    """2.1 M samples with the BERT statistics (key 6) and the diagnostic log (key 9) on: every log entry == the oracle's, the PRBS9 counts ==
    the oracle's receiver over the oracle's BERT frames, no deferred-cost tag is left in any viterbi_cost (bit 31 only in -1), and the
    device compaction and a truncated fetch deliver the same records."""
    import torch
    x, per, diags, logs, stats, room = _consumers_case()
    Cn, T = x.shape
    exp = np.concatenate(per)
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.tune(6, 1)
        ctx.tune(9, room)
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got = ctx.frames()
        d = ctx.diag(Cn)
        glog = ctx.diag_log(Cn, capacity=room)
        st = ctx.bert_stats(Cn)
        part = np.zeros(1000, dtype=m17hip.FRAME_REC)
        n = C.c_uint64(0)
        code = ctx.lib.m17hip_frames_fetch(ctx.h, part.ctypes.data_as(C.c_void_p), C.c_uint64(part.size), C.byref(n))
        assert code == m17hip.ETRUNC and n.value == exp.size and part.tobytes() == exp[:1000].tobytes()
        with torch.cuda.stream(ctx.torch_stream()):
            dev = torch.full((exp.size + 8, 64), 0xEE, dtype=torch.uint8, device="cuda")
            nd = ctx.frames_compact_device(dev.data_ptr(), exp.size + 8)
            compact = dev[:nd].cpu().numpy()
        assert nd == exp.size and compact.tobytes() == exp.tobytes()
    finally:
        ctx.close()
    _assert_records(got, per, "consumers")
    _assert_diag(d, diags, "consumers")
    for c in range(Cn):
        assert glog[c].size == logs[c].size, (c, glog[c].size, logs[c].size)
        if glog[c].tobytes() != logs[c].tobytes():
            bad = np.flatnonzero((_rows64(glog[c]) != _rows64(logs[c])).any(axis=1))
            i = int(bad[0])
            raise AssertionError(f"diagnostic log of channel {c}: {bad.size} of {logs[c].size} entries differ, first at {i} in "
                                 f"{[f for f in logs[c].dtype.names if not np.array_equal(glog[c][i][f], logs[c][i][f], equal_nan=f in FLOAT_FIELDS)]}")
        for costs in (glog[c]["viterbi_cost"], d["viterbi_cost"][c:c + 1]):
            assert ((costs >= 0) | (costs == -1)).all(), c       # settled costs: bit 31 only in -1
        bits, errs, sync = stats[c]
        frames = int((per[c]["frame_type"] == 5).sum())
        assert (int(st["bits"][c]), int(st["errors"][c]), bool(st["synced"][c]), int(st["frames"][c])) == (bits, errs, sync, frames), c


# ------------------------------------------------------------------------------------------------ 7: per-operator entry points ---
@pytest.mark.parametrize("Cn,short", [(1, 0), (2, 0), (1, 1)], ids=["C1_L", "C2_L", "C1_L-1"])
def test_operators_at_the_limit(limit, Cn, short):
    """m17hip_fir_rrc150, m17hip_correlator, m17hip_fir_correlator and m17hip_dcd on whole rows of L (and L - 1) samples: every value of
    every row against the oracle; of the K3 table the sums since the start (index 5) at the last tick and at 64 random ticks per channel,
    and the restarted sums (index start % 5) at 16 more."""
    T = L - short
    x = np.ascontiguousarray(limit.x[:Cn, :T])
    exp_y = _par(ol.fir_i16, [x[c] for c in range(Cn)])
    exp_lk = _par(ol.correlator, exp_y)
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.upload(x)
        y = ctx.fir()
        for c in range(Cn):
            _assert_row_equal(y[c], exp_y[c], f"fir row {c}")
        del y
        limit_, corr = ctx.correlator()
        for c in range(Cn):
            _assert_row_equal(limit_[c], exp_lk[c][0], f"correlator: limit row {c}")
            for j in range(4):
                _assert_row_equal(corr[j, c], exp_lk[c][1][j], f"correlator: corr {j} row {c}")
        del limit_, corr
        y, limit_, corr = ctx.fir_correlator()
        for c in range(Cn):
            _assert_row_equal(y[c], exp_y[c], f"fir_correlator: y row {c}")
            _assert_row_equal(limit_[c], exp_lk[c][0], f"fir_correlator: limit row {c}")
            for j in range(4):
                _assert_row_equal(corr[j, c], exp_lk[c][1][j], f"fir_correlator: corr {j} row {c}")
        del y, limit_, corr, exp_y, exp_lk
        sums = ctx.dcd()
    finally:
        ctx.close()
    ticks = T // 192
    assert sums.shape == (Cn, ticks, 2, 6) and ticks > 174000
    rng = np.random.default_rng(7 + Cn + short)
    checks = []
    for c in range(Cn):
        for k in [ticks - 1] + [int(v) for v in rng.integers(12, ticks, 64)]:
            checks.append((c, k, 5, 0, 192 * (k + 1)))
        for k in [ticks - 1] + [int(v) for v in rng.integers(12, ticks, 15)]:
            span = int(rng.choice([1, 2, 3, 5]))
            a0 = k - span + 1
            checks.append((c, k, a0 % 5, 192 * a0, 192 * span))
    xs = [ol.scale(x[c]) for c in range(Cn)]
    exp_s = _par(lambda q: ol.dcd_sums(xs[q[0]], q[3], q[4]), checks)
    for (c, k, j, _, _), e in zip(checks, exp_s):
        assert (float(sums[c, k, 0, j]), float(sums[c, k, 1, j])) == (float(e[0]), float(e[1])), (c, k, j)


# ------------------------------------------------------------------------------------------------ 8: device synthesis ------------
@pytest.mark.parametrize("chan0", [0, 1000003])
def test_device_synthesis_at_the_limit(limit, chan0):
    """m17hip_synth_i16 at T = L with 17 469 payload frames per channel (the symbol buffer at its largest): every int16 against the test
    generator, for the first channels of the job and for channels a million further on."""
    Cn = 3
    exp = limit.x[:Cn] if chan0 == 0 else ol.generate_batch(limit.params, Cn, L, threads=THREADS, chan0=chan0)
    assert limit.params.n_frames == L // 1920 - 6 > 17000
    ctx = m17hip.Context(Cn, L)
    try:
        ctx.synth(limit.params, Cn, L, chan0=chan0)
        got = ctx.download()
    finally:
        ctx.close()
    assert np.array_equal(got, exp), (chan0, int((got != exp).sum()), np.flatnonzero((got != exp).any(axis=0))[:4].tolist())
