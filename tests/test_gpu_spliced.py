"""GPU: transmissions joined late, cut short, with holes and with an overwritten LSF (tests/spliced.py).  Every other input of the suite is whole and well-formed,
so three parts of the state machine that the sequential kernel and the deferred decode reproduce were reached by luck only: a sync word accepted
without a preamble (the second half of do_unlocked), the frame decoder's walk from its LSF state through six LICH segments to an assembled LSF and
on to STREAM — where the set of frames that may be decoded later, one lane per frame, changes — and the missing-sync counting of a carrier that
disappears without EOT.  A packet transmission joined late is reported as LICH and BERT records, since the packet sync word negated is the BERT one.

Everything is compared with the oracle bit for bit, no tolerance anywhere: records as bytes, every integer and float field of m17_diag, and every
callback of the diagnostic log.  tests/test_spliced.py asserts on the oracle alone, on every channel, that these very inputs reach those paths."""
import numpy as np
import pytest

import m17hip
import off_clock as oc
import oracle_lib as ol
import spliced as sp

pytestmark = pytest.mark.gpu

INT_FIELDS = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock", "dcd_level")
Cn, T = sp.C, sp.T
ROOM = T // 384 + 2


# the three configurations of tests/test_gpu_parity.py's ctx fixture (keys 15, 10, 20, 17), and the decode in K5 with the EVM fold outside it
@pytest.fixture(scope="module", params=[(1, -1, 0, 1), (0, -1, 0, 0), (1, 1, 1, 1), (0, -1, 0, 1)],
                ids=["default", "decode_and_evm_in_k5", "k3_latency_form_redo_in_front", "decode_in_k5_evm_outside"])
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


def _check_diag(d, diags, what):
    for f in INT_FIELDS:
        assert np.array_equal(d[f], diags[f]), (what, f, np.flatnonzero(d[f] != diags[f])[:16].tolist())
    for f in FLOAT_FIELDS:
        same = (d[f].view(np.uint32) == diags[f].view(np.uint32)) | (np.isnan(d[f]) & np.isnan(diags[f]))
        assert same.all(), (what, f, np.flatnonzero(~same)[:16].tolist())


def _check(got, d, rows, diags, what, glog=None, logs=None):
    e = np.concatenate(rows)
    if got.tobytes() != e.tobytes():
        bad = [c for c in range(len(rows)) if got[got["channel"] == c].tobytes() != rows[c].tobytes()]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {e.size} expected), channels {bad[:24]}")
    _check_diag(d, diags, what)
    if glog is not None:
        for c in range(len(rows)):
            if glog[c].tobytes() != logs[c].tobytes():
                n = min(glog[c].size, logs[c].size)
                k = next((i for i in range(n) if glog[c][i].tobytes() != logs[c][i].tobytes()), n)
                raise AssertionError(f"{what}: diagnostic log of channel {c} differs at callback {k} of {glog[c].size} / {logs[c].size}: "
                                     f"{glog[c][k] if k < glog[c].size else None} / {logs[c][k] if k < logs[c].size else None}")


# ---- one shot, in place ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sp.BATCHES)
def test_one_run_records_diagnostics_and_every_callback(ctx, name):
    """64 channels x 96 000 samples of each batch under each schedule setting: records, m17_diag and the whole diagnostic log of every channel."""
    x, rows, diags, logs = sp.rows_of(name)
    ctx.tune(9, ROOM)
    try:
        ctx.upload(x); ctx.reset(); ctx.run()
        got, d, glog = ctx.frames().copy(), ctx.diag(Cn), ctx.diag_log(Cn, capacity=ROOM)
    finally:
        ctx.tune(9, 0)
    assert got.size > 10 * Cn
    _check(got, d, rows, diags, f"one run, {name}", glog, logs)


# ---- a run boundary inside the LICH collection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sp.RUN_KINDS)
@pytest.mark.parametrize("name", ["late", "blank"])
def test_run_boundaries_inside_the_lich_collection(ctx, name, kind):
    """The stream as consecutive in-place runs shorter than the 9600 samples a collection spans at least, so it lies astride a boundary on every
    stream channel (tests/test_spliced.py).  The records joined over the runs equal the one-shot oracle's; m17_diag after EVERY run equals an
    oracle demodulator fed the same prefix."""
    x, rows, diags, logs = sp.rows_of(name)
    lengths, expected = sp.run_lengths(kind), sp.prefix_diags(name, kind)
    assert sum(lengths) == T
    ctx.reset()
    parts, pos = [], 0
    for n, dp in zip(lengths, expected):
        ctx.upload(x[:, pos:pos + n]); ctx.run()
        parts.append(ctx.frames().copy())
        pos += n
        _check_diag(ctx.diag(Cn), dp, f"{name}, {kind}: m17_diag after {pos} samples")
    _check(_sorted(parts), ctx.diag(Cn), rows, diags, f"{name}, {kind}")


# ---- per-channel polarity crossed in -----------------------------------------------------------------------------------------------------------
def test_late_entry_under_a_mixed_polarity_table(cfg):
    """Every second channel from an inverted transmitter, with a polarity table that says so: the direct acceptance in do_unlocked tells LSF from
    STREAM and packet from BERT by the sign alone, so a polarity slip changes the KIND of record."""
    y, pol = sp.late_mixed_polarity()
    rows, diags, logs = oc.oracle_of("spliced late, mixed polarity", y, pol, logs=True)
    c = _open(cfg)
    try:
        c.set_channel_polarity(pol)
        c.tune(9, ROOM)
        c.upload(y); c.reset(); c.run()
        _check(c.frames().copy(), c.diag(Cn), rows, diags, "late entry, mixed polarity", c.diag_log(Cn, capacity=ROOM), logs)
    finally:
        c.close()


# ---- the same as a staged live feed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["fetch_then_run", "run_then_fetch"])
@pytest.mark.parametrize("name", ["late", "blank"])
def test_staged_live_feed_across_the_lich_collection(ctx, name, order):
    """The call sequence of tests/test_gpu_streaming.py's _pipelined, both call orders, ten runs of 9600 samples: the records of run k are fetched
    after run k + 1 was queued, while the frame-decoder state crosses LSF -> STREAM."""
    import torch
    x, rows, diags, logs = sp.rows_of(name)
    L = 9600
    n = T // L
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
    _check(_sorted(parts), ctx.diag(Cn), rows, diags, f"staged, {name}, {order}")


# ---- a channel reset in the middle of the collection ----------------------------------------------------------------------------------------------
def test_reset_channels_in_the_middle_of_the_lich_collection(cfg):
    """Runs of 4800 samples; every third late-entry stream gets a fresh demodulator behind the run that holds its third LICH record
    (spliced.reset_plan, from the oracle's positions).  From there on it reports what a fresh oracle demodulator started at that sample reports
    — the collection starts over, seq from 0 — and the untouched channels what the oracle reports over the whole stream.  Compared run by run."""
    x, rows, diags, logs = sp.rows_of("late")
    fresh = sp.reset_expectation()
    L = 4800
    exp_diags = diags.copy()
    for ch, (at, r, d) in fresh.items():
        exp_diags[ch] = d
    c = _open(cfg)
    try:
        c.reset()
        for k in range(T // L):
            lo, hi = k * L, (k + 1) * L
            todo = [ch for ch, (at, _, _) in fresh.items() if at == lo]
            if todo:
                c.reset_channels(todo)
            c.upload(x[:, lo:hi]); c.run()
            got = c.frames().copy()
            exp = []
            for ch in range(Cn):
                if ch in fresh and fresh[ch][0] <= lo:
                    at, r = fresh[ch][0], fresh[ch][1]
                    exp.append(r[(r["sample_pos"] + at >= lo) & (r["sample_pos"] + at < hi)])
                else:
                    exp.append(rows[ch][(rows[ch]["sample_pos"] >= lo) & (rows[ch]["sample_pos"] < hi)])
            if got.tobytes() != np.concatenate(exp).tobytes():
                bad = [ch for ch in range(Cn) if got[got["channel"] == ch].tobytes() != exp[ch].tobytes()]
                raise AssertionError(f"run {k}: records differ, channels {bad[:24]} (reset: {sorted(fresh)})")
        _check_diag(c.diag(Cn), exp_diags, "after the last run")
    finally:
        c.close()


# ---- consumers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["late", "splice"])
def test_consumers_on_head_cut_and_spliced_channels(cfg, name):
    """m17hip_bert_stats and m17hip_packets_fetch against the CPU consumers fed the oracle's records (tests/test_gpu_channel_reset.py's way), two runs:
    a packet whose LSF or first frames were cut yields what the CPU consumer yields, nothing included."""
    x, rows, diags, logs = sp.rows_of(name)
    c = _open(cfg)
    try:
        c.tune(6, 1)
        c.tune(7, 1024)
        c.reset()
        pk = []
        for a, b in ((0, 40007), (40007, T)):
            c.upload(x[:, a:b]); c.run()
            pk.append(c.packets().copy())
        st = c.bert_stats(Cn)
        got = np.concatenate(pk)
    finally:
        c.close()
    n_packets = 0
    for ch in range(Cn):
        r = rows[ch]
        pay = r[r["frame_type"] == sp.FT_BERT]["payload"][:, :25]
        bits, errs, sync = ol.bert_count(pay) if pay.size else (0, 0, False)
        assert (int(st["bits"][ch]), int(st["errors"][ch]), bool(st["synced"][ch]), int(st["frames"][ch])) == (bits, errs, sync, pay.shape[0]), ch
        exp = ol.PacketAssembler().feed(r["frame_type"], r["payload"]) if r.size else []
        g = got[got["channel"] == ch]
        assert len(exp) == g.size, (ch, len(exp), g.size)
        for e, q in zip(exp, g):
            assert (int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"])) == (e["size"], e["checksum"], e["frames"], e["seq_errors"]), ch
            assert np.array_equal(q["data"], e["data"]) and int(q["sample_pos"]) == int(r["sample_pos"][e["rec_index"]]), ch
        n_packets += len(exp)
    if name == "late":
        assert n_packets == 0          # head-cut packets are never reported as packet frames (spliced.PACKET_HIST)


def test_lsf_info_of_the_lsfs_assembled_from_lich(ctx):
    """The LSF records assembled from LICH on the late-entry channels through m17hip_lsf_info: the transmitted LSF's info, from the generator's truth."""
    x, rows, diags, logs = sp.rows_of("late")
    meta = sp.batch("late")["meta"]
    chans = [ch for ch in range(Cn) if meta[ch]["kind"] == 1]
    ctx.upload(x); ctx.reset(); ctx.run()
    got = ctx.frames().copy()
    batch = []
    for ch in chans:
        g = got[got["channel"] == ch]
        batch.append(g[sp.assembled_lsf(g)[0]]["payload"][:30])
    info = ctx.lsf_info(np.stack(batch))
    for i, ch in enumerate(chans):
        f = meta[ch]["lsf"]
        assert bytes(batch[i]) == bytes(f), ch
        assert bytes(info["dst"][i]).ljust(10, b"\0") == ol.decode_callsign(f[0:6]) and bytes(info["src"][i]).ljust(10, b"\0") == ol.decode_callsign(f[6:12]), ch
        assert int(info["type"][i]) == (int(f[12]) << 8 | int(f[13])) and bool(info["crc_ok"][i]), ch


# ---- one long case ----------------------------------------------------------------------------------------------------------------------------------
def test_long_stream_joined_late_with_holes_across_segment_boundaries():
    """8 channels x 480 000 samples in one run of ten default segments, default knobs: the LICH collection and each of three holes lie astride a
    48 000-sample segment boundary (tests/test_spliced.py); records, m17_diag and the whole diagnostic log."""
    x, rows, diags, logs = sp.long_rows()
    room = sp.LONG_T // 384 + 2
    c = m17hip.Context(sp.LONG_C, sp.LONG_T)
    try:
        c.tune(9, room)
        c.upload(x); c.reset(); c.run()
        _check(c.frames().copy(), c.diag(sp.LONG_C), rows, diags, "long case", c.diag_log(sp.LONG_C, capacity=room), logs)
    finally:
        c.close()
