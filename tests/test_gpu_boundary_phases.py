"""GPU: one run or segment boundary at every phase of the frame cycle (tests/boundary_phases.py: channel c carries the same transmission delayed by c
samples, 1920 channels).  The sequential kernel works in chunks — a locked frame in two, the sync phase as 77 counting samples plus a nine-sample window,
48 symbols of LSF_SYNC, 480 samples of the unlocked search — and the host cuts streams into runs and runs into segments; what crosses such a cut (a
trigger that is still up, a pending clock update, the ring, the counts, a half-filled framer, a deferred frame's reserved record, K2's boundary copy, the
carried tails) is state that has to be saved and found again.  Here every cut meets every phase on some channel of the batch.

Everything is compared with the oracle bit for bit: frame records as bytes, every callback of the diagnostic log (floats as words, NaN for NaN) and the
final m17_diag.  Where the stream is fed in runs the PARTITION is asserted as well: the records and log entries of run k are exactly the oracle's for that
run's samples, so a frame reported one run early or late fails (joining the runs and sorting them would not show it).  tests/test_boundary_phases.py
asserts on the oracle alone that these inputs put a frame completion, and with it everything at a fixed offset from one, on every phase."""
import numpy as np
import pytest

import boundary_phases as bp
import f32_lib as fl
import m17hip
import oracle_lib as ol
import voice_log as vl

pytestmark = pytest.mark.gpu

Cn, T = bp.C, bp.T
ROOM_RUN, ROOM_ALL = 8, T // 384 + 2          # diagnostic callbacks of room: a run of 1920 samples fires five at the most
INT_FIELDS = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock", "dcd_level")
DEFAULTS = {3: 48000, 33: -1, 26: -1, 15: 1, 17: 1, 9: 0, 6: 0, 7: 0, 34: 0}
VOICE_ROOM, PACKET_ROOM = 8, 4096


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(Cn, T)
    yield c
    c.close()


class knobs:
    """m17hip_tune keys for the length of a with block; every key goes back to its default behind it."""

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.tune(k, v)

    def __exit__(self, *exc):
        if exc[0] is not None:          # a failed test may leave a staged input or a queued front end behind: a reset abandons both
            self.ctx.upload_wait()
            self.ctx.reset()
        for k in self.kv:
            self.ctx.tune(k, DEFAULTS[k])


def _form(x, dtype):
    return bp.f32(x) if dtype == "float32" else x


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------------
def _diag_mismatch(got, exp, fields=INT_FIELDS + ("pad",)):
    """None when two m17_diag arrays agree (integers equal, floats equal as words or both NaN), else (field, indices)."""
    if got.tobytes() == exp.tobytes():
        return None
    if got.size != exp.size:
        return "size", [got.size, exp.size]
    for f in fields:
        bad = got[f] != exp[f]
        if bad.any():
            return f, np.flatnonzero(bad.reshape(got.size, -1).any(axis=1))[:16].tolist()
    for f in FLOAT_FIELDS:
        same = (got[f].view(np.uint32) == exp[f].view(np.uint32)) | (np.isnan(got[f]) & np.isnan(exp[f]))
        if not same.all():
            return f, np.flatnonzero(~same)[:16].tolist()
    return None


def _check_records(got, exp, what):
    if got.tobytes() != exp.tobytes():
        chans = np.union1d(got["channel"], exp["channel"])
        bad = [int(c) for c in chans if got[got["channel"] == c].tobytes() != exp[exp["channel"] == c].tobytes()]
        c = bad[0]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {exp.size} expected) on {len(bad)} channels {bad[:16]}; channel {c}: "
                             f"{got[got['channel'] == c][['seq', 'sample_pos', 'frame_type', 'cost']].tolist()} / "
                             f"{exp[exp['channel'] == c][['seq', 'sample_pos', 'frame_type', 'cost']].tolist()}")


def _check_log(glog, exp, counts, what):
    n = np.array([l.size for l in glog], dtype=np.uint32)
    if not np.array_equal(n, counts):
        bad = np.flatnonzero(n != counts)
        raise AssertionError(f"{what}: callbacks per channel differ on {bad.size} channels {bad[:16].tolist()}: {n[bad[:16]].tolist()} / {counts[bad[:16]].tolist()}")
    m = _diag_mismatch(np.concatenate(glog), exp)
    if m is not None:
        chan = np.repeat(np.arange(len(glog)), n)
        raise AssertionError(f"{what}: diagnostic log differs in {m[0]}, channels {np.unique(chan[m[1]]).tolist() if m[0] != 'size' else m[1]}")


def _check_final(ctx, o, what):
    m = _diag_mismatch(ctx.diag(o.C), o.diags, INT_FIELDS)
    assert m is None, f"{what}: final m17_diag differs in {m[0]}, channels {m[1]}"


def _rows_of(recs, channels):
    """The records of one piece (in channel order) as one array per channel."""
    cut = np.searchsorted(recs["channel"], np.arange(channels + 1))
    return [recs[cut[c]:cut[c + 1]] for c in range(channels)]


class Consumers:
    """The consumers that carry state from run to run, beside the runs of one stream: the CPU twins (tests/voice_log.py, ol.PacketAssembler, ol.bert_count)
    fed the oracle's records of the same runs.  A call or a packet is reported once, by the run that closes it."""

    def __init__(self, channels):
        self.C = channels
        self.voice = vl.VoiceBank(channels)
        self.asm = [ol.PacketAssembler() for _ in range(channels)]
        self.bert = [[] for _ in range(channels)]
        self.calls = self.packets = 0

    def check_run(self, ctx, recs, what):
        rows = _rows_of(recs, self.C)
        audio, marks, counts, calls = self.voice.feed(rows)
        ga, gm, gn = ctx.voice(channels=self.C)
        gc = ctx.calls(capacity=self.C * m17hip.calls_per_channel(VOICE_ROOM))
        assert np.array_equal(gn, counts), (what, "voice counts", np.flatnonzero(gn != counts)[:16].tolist())
        used = np.arange(ga.shape[1])[None, :] < counts[:, None]
        assert np.array_equal(gm[used], marks[:, :ga.shape[1]][used]) and np.array_equal(ga[used], audio[:, :ga.shape[1]][used]), (what, "voice planes")
        assert gc.size == calls.size and gc.tobytes() == calls.tobytes(), (what, "calls", gc.size, calls.size)
        self.calls += calls.size
        got = ctx.packets(capacity=PACKET_ROOM)
        exp = []
        for c in np.unique(recs["channel"]).tolist():
            r = rows[c]
            for e in self.asm[c].feed(r["frame_type"], r["payload"]):
                exp.append((c, e["size"], e["checksum"], e["frames"], e["seq_errors"], int(r["sample_pos"][e["rec_index"]]), e["data"]))
            pay = r[r["frame_type"] == bp.FT_BERT]["payload"][:, :25]
            if pay.size:
                self.bert[c].append(pay)
        assert got.size == len(exp), (what, "packets", got.size, len(exp))
        for q, e in zip(got, exp):
            assert (int(q["channel"]), int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"]), int(q["sample_pos"])) == e[:6], (what, e[:6])
            assert np.array_equal(q["data"], e[6]), (what, e[0])
        self.packets += len(exp)

    def check_bert(self, ctx, what):
        st = ctx.bert_stats(self.C)
        for c in range(self.C):
            pay = np.concatenate(self.bert[c]) if self.bert[c] else np.zeros((0, 25), dtype=np.uint8)
            bits, errs, sync = ol.bert_count(pay) if pay.size else (0, 0, False)
            assert (int(st["bits"][c]), int(st["errors"][c]), bool(st["synced"][c]), int(st["frames"][c])) == (bits, errs, sync, pay.shape[0]), (what, c)


# ---- the ways a stream is fed --------------------------------------------------------------------------------------------------------------------
def _in_runs(ctx, name, L, dtype="int16", consumers=False, what=None):
    """The stream in consecutive in-place runs of L samples: per run the records and the diagnostic log are the oracle's for that run's samples."""
    o, x = bp.oracle(name), bp.batch(name)
    what = what or f"{name}, runs of {L}, {dtype}"
    ends = bp.run_ends(L)
    recs, logs, counts = o.pieces(ends)
    cons = Consumers(o.C) if consumers else None
    ctx.reset()
    for k, e in enumerate(ends.tolist()):
        chunk = x[:, e - L:e]
        ctx.upload(fl.on_grid(chunk) if dtype == "float32" else chunk)
        ctx.run()
        _check_records(ctx.frames(), recs[k], f"{what}, run {k}")
        _check_log(ctx.diag_log(o.C, capacity=ROOM_RUN), logs[k], counts[k], f"{what}, run {k}")
        if cons:
            cons.check_run(ctx, recs[k], f"{what}, run {k}")
            if k in (len(ends) // 2, len(ends) - 1):
                cons.check_bert(ctx, f"{what}, after run {k}")
    _check_final(ctx, o, what)
    return cons


def _in_segments(ctx, name, dtype="int16", what=None):
    """The stream in ONE run (the segment length is the caller's knob): records, the whole diagnostic log and the final m17_diag."""
    o = bp.oracle(name)
    what = what or f"{name}, one run, {dtype}"
    ctx.reset()          # (first: a stream's sample format is free again only behind a reset)
    ctx.upload(_form(bp.batch(name), dtype))
    ctx.run()
    _check_records(ctx.frames(), o.recs, what)
    _check_log(ctx.diag_log(o.C, capacity=ROOM_ALL), o.log, np.array([l.size for l in o.logs], dtype=np.uint32), what)
    _check_final(ctx, o, what)
    # K2's redo (the pass that takes a channel up again from its boundary record) did run: a forced unlock takes the channel off the limit-filter replay,
    # so at least every channel whose forced unlock the oracle's log shows has left it once
    forced = np.unique(o.forced_unlocks()[0]).size
    drops = ctx.replay_drops()
    print(f"{what}: {drops} replay drops, {forced} channels with a forced unlock")
    assert drops >= forced > 0, (what, drops, forced)


# ---- a, b: runs of 1920 and of 640 samples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", bp.BATCHES)
def test_runs_of_a_frame(ctx, name, dtype):
    """upload + run + fetch every 1920 samples: the run boundary falls on every sample of the frame cycle on some channel.  On the int16 feed the consumers
    that carry state from run to run (voice planes and call log, packet reassembly, BERT statistics) run beside it and are held against their CPU twins."""
    cons = dtype == "int16"
    with knobs(ctx, k9=ROOM_RUN, **({"k34": VOICE_ROOM, "k7": PACKET_ROOM, "k6": 1} if cons else {})):
        c = _in_runs(ctx, name, 1920, dtype, consumers=cons)
    if cons and name == "stream":
        assert c.calls >= Cn // 2          # (the consumers had something to carry: calls closed, packets completed)
    if cons and name == "packet":
        assert c.packets >= Cn // 4          # (the even channels send a whole packet)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", bp.BATCHES)
def test_runs_of_a_third_of_a_frame(ctx, name, dtype):
    """Runs of 640 samples: the 960-sample carrier-detect point meets the run boundary at three offsets, not one."""
    with knobs(ctx, k9=ROOM_RUN):
        _in_runs(ctx, name, 640, dtype)


# ---- c, d: one run, segments of 1920 and of 640 samples ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [1920, 640])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", bp.BATCHES)
def test_segments_of_a_frame_and_of_a_third(ctx, name, dtype, seg):
    """One run of 24 frames cut into K2 / K5 segments of `seg` samples (no ramp): the segment boundary on every phase."""
    with knobs(ctx, k9=ROOM_ALL, k3=seg, k33=0):
        _in_segments(ctx, name, dtype, f"{name}, segments of {seg}, {dtype}")


@pytest.mark.parametrize("seg", [1920, 640])
def test_gate_aware_front_end_across_segments(ctx, seg):
    """The same with the gate-aware front end (the matched filter follows K5 of segment k - 2 and skips what the forecast says the carrier is off for) on
    the packet batch.  Cut every 640 samples every channel has segments to skip, in front of the transmission; cut every 1920 none has, and the cell runs
    the gate-aware schedule with nothing to skip (tests/test_boundary_phases.py asserts both on the oracle's log)."""
    with knobs(ctx, k9=ROOM_ALL, k3=seg, k33=0, k26=1):
        _in_segments(ctx, "packet", "int16", f"packet, gate-aware, segments of {seg}")


# ---- e: a staged live feed ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
@pytest.mark.parametrize("name", ["stream", "bert"])
def test_staged_runs_of_a_frame(ctx, name, order):
    """Runs of 1920 samples staged from pinned memory with the front end queued ahead — the call sequence of tests/test_gpu_streaming.py's _pipelined, both
    orders.  The diagnostic log is the latest run's: in the first order that is run k when its records are fetched, in the second run k + 1."""
    import torch
    o, x, L = bp.oracle(name), bp.batch(name), 1920
    ends = bp.run_ends(L)
    n = ends.size
    recs, logs, counts = o.pieces(ends)
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, k * L:(k + 1) * L])).pin_memory() for k in range(n)]
    what = f"staged, {name}, {order}"

    def log_of(k):
        _check_log(ctx.diag_log(Cn, capacity=ROOM_RUN), logs[k], counts[k], f"{what}, run {k}")

    with knobs(ctx, k9=ROOM_RUN):
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), Cn, L)
        ctx.run(channels=Cn, samples=L)
        if order == "run_then_fetch":
            log_of(0)
        for k in range(n):
            if k + 1 < n:
                ctx.upload_async(pins[k + 1].data_ptr(), Cn, L)
                ctx.front(channels=Cn, samples=L)
                if order == "run_then_fetch":
                    ctx.run(channels=Cn, samples=L)
                    ctx.frames_select(1)
            _check_records(ctx.frames(), recs[k], f"{what}, run {k}")
            ctx.frames_select(0)
            if order == "run_then_fetch":
                if k + 1 < n:
                    log_of(k + 1)
            else:
                log_of(k)
                if k + 1 < n:
                    ctx.run(channels=Cn, samples=L)
        ctx.upload_wait()
        _check_final(ctx, o, what)


# ---- f: the other forms of the decode and of the EVM fold ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feed", ["runs_of_1920", "segments_of_1920", "segments_of_640"])
@pytest.mark.parametrize("form", ["decode_in_k5", "evm_in_k5"])
@pytest.mark.parametrize("name", ["stream", "bert"])
def test_decode_and_evm_fold_inside_the_sequential_kernel(ctx, name, form, feed):
    """Key 15 = 0 (every frame decoded where it completes: no deferred frame's reserved record crosses the cut) and key 17 = 0 (the EVM folded inside K5)."""
    kv = {"k15": 0} if form == "decode_in_k5" else {"k17": 0}
    if feed == "runs_of_1920":
        with knobs(ctx, k9=ROOM_RUN, **kv):
            _in_runs(ctx, name, 1920, what=f"{name}, {form}, runs of 1920")
    else:
        seg = int(feed.rsplit("_", 1)[1])
        with knobs(ctx, k9=ROOM_ALL, k3=seg, k33=0, **kv):
            _in_segments(ctx, name, what=f"{name}, {form}, segments of {seg}")


# ---- g: per-channel polarity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_runs_of_a_frame_under_a_mixed_polarity_table(ctx, dtype):
    """384 channels, every second one from an inverted transmitter and marked so in the polarity table."""
    try:
        ctx.set_channel_polarity(bp.polarity())
        with knobs(ctx, k9=ROOM_RUN):
            _in_runs(ctx, "mixed", 1920, dtype)
    finally:
        ctx.set_channel_polarity(None)


# ---- h: do_packet_sync gives up ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feed", ["runs_of_1920", "segments_of_1920"])
def test_packet_sync_gives_up_across_a_boundary(ctx, feed):
    """The packet-hole batch: on a third of its channels eleven sync words go missing at a cost of 60 or more and the demodulator leaves PACKET_SYNC for
    UNLOCKED with a forced dcd.unlock() (tests/test_boundary_phases.py), at every fifth phase of the boundary."""
    if feed == "runs_of_1920":
        with knobs(ctx, k9=ROOM_RUN):
            _in_runs(ctx, "hole", 1920)
    else:
        with knobs(ctx, k9=ROOM_ALL, k3=1920, k33=0):
            _in_segments(ctx, "hole", what="hole, segments of 1920")
