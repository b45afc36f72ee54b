"""GPU tests of m17hip_demod_reset_channels (include/m17hip.h): fresh demodulators for SOME channels of a context between the runs of a stream.
The reference's answer to a retuned receiver or a source that came back is a new m17-demod process for that one stream; so, for a channel
reset in front of run k of a stream cut into runs of T samples, the library must report

  * before the reset what the oracle reports over x[:k T] — the reset takes nothing back,
  * from the reset on what a FRESH oracle demodulator reports over x[k T:], seq / sample_pos / n_frames / n_diag counted from zero,
  * and for every channel that was not reset what the oracle reports over the whole stream (tests/test_gpu_streaming.py),

all of it bit for bit: records, m17_diag (evm included), the diagnostic log, BERT statistics, packets."""
import concurrent.futures
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
THREADS = 16
T = 24000   # samples per run: 125 carrier-detect ticks of 192 samples
# m17_diag of a continued stream, the fields tests/test_gpu_streaming.py compares (evm included); the diagnostic log is compared whole
INT_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock")


def _par(fn, items):
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(fn, items))


def _stream(Cn, total, seed, sigma=600.0):
    """Channel c: BERT (c % 3 == 0), voice-like stream (1) — one transmission over the whole stream, so that every run boundary lies inside it —
    or packets closed by an FCS (2): a transmission of 16 frames every 48 000 samples (two runs), each behind its own loud lead-in as the first one
    is, so that odd run boundaries fall inside a packet and even ones between two."""
    x = np.zeros((Cn, total), dtype=np.int16)
    for kind, first in ((0, 0), (1, 1)):
        rows = np.arange(first, Cn, 3)
        p = ol.gen_params(seed=seed + kind, kind=kind, n_frames=total // 1920 - 4, lead_in=3072, noise_sigma=sigma, tail_sigma=sigma,
                          lead_sigma=40000.0, total=total)
        x[rows] = ol.generate_batch(p, rows.size, total, threads=THREADS, chan0=first)
    for c in range(2, Cn, 3):
        for i, pos in enumerate(range(0, total, 2 * T)):
            n = min(2 * T, total - pos)
            p = ol.gen_params(seed=seed + 1000 * c + i, kind=4, n_frames=16, lead_in=3072, noise_sigma=sigma, tail_sigma=sigma, lead_sigma=40000.0,
                              total=n)
            x[c, pos:pos + n] = ol.generate(p)[:n]
    return x


def _origins(Cn, n_runs, resets):
    """a[r][c]: the run at whose start channel c's demodulator of run r began (0, or its latest reset at or before r)."""
    a = np.zeros((n_runs, Cn), dtype=np.int64)
    cur = np.zeros(Cn, dtype=np.int64)
    for r in range(n_runs):
        for c in resets.get(r, ()):
            cur[c] = r
        a[r] = cur
    return a


def _expect(x, n_runs, resets, logs=False, runs=None, T=T):
    """Per run r: the oracle's records of that run (flat, ordered by (channel, seq)), its m17_diag of every channel at the end of the run, and (logs)
    every diagnostic callback of the run per channel — each channel demodulated by a fresh oracle from its latest reset to the end of run r."""
    Cn = x.shape[0]
    org = _origins(Cn, n_runs, resets)
    out = []
    for r in (range(n_runs) if runs is None else runs):
        rows = [None] * Cn
        diags = np.zeros(Cn, dtype=ol.DIAG)
        lg = [None] * Cn
        for a in np.unique(org[r]):
            chs = np.flatnonzero(org[r] == a)
            seg = np.ascontiguousarray(x[chs, a * T:(r + 1) * T])
            recs, counts, d = ol.demod_batch(seg, cap=2 * (seg.shape[1] // 1920 + 2) + 4, threads=THREADS)
            first = (r - a) * T
            for i, c in enumerate(chs):
                rc = recs[i, : counts[i]]
                rc = rc[rc["sample_pos"] >= first].copy()
                rc["channel"] = c
                rows[c] = rc
                diags[c] = d[i]
            if logs:
                room = seg.shape[1] // 384 + 2
                for c, full in zip(chs, _par(lambda i: ol.demod_diag_log(seg[i], cap=room), range(chs.size))):
                    pos = full["pad"][:, 0].astype(np.uint64) | (full["pad"][:, 1].astype(np.uint64) << np.uint64(32))
                    lg[c] = full[pos >= first].copy()
        out.append((rows, diags, lg))
    return out


def _flat(rows):
    return np.concatenate(rows)


def _assert_run(got, d, exp, what, glog=None):
    rows, diags, lg = exp
    e = _flat(rows)
    if got.tobytes() != e.tobytes():
        bad = [c for c in range(len(rows)) if got[got["channel"] == c].tobytes() != rows[c].tobytes()]
        raise AssertionError(f"{what}: records differ ({got.size} fetched / {e.size} expected), channels {bad[:24]}")
    if d is not None:
        for f in INT_FIELDS:
            assert np.array_equal(d[f], diags[f]), (what, f, np.flatnonzero((d[f] != diags[f]).reshape(len(d), -1).any(axis=1))[:16].tolist())
        for f in FLOAT_FIELDS:
            assert np.array_equal(d[f], diags[f], equal_nan=True), (what, f, np.flatnonzero(~((d[f] == diags[f]) | (np.isnan(d[f]) & np.isnan(diags[f]))))[:16].tolist())
    if glog is not None:
        for c in range(len(rows)):
            assert glog[c].tobytes() == lg[c].tobytes(), (what, "diagnostic log", c, glog[c].size, lg[c].size)


def _in_place(ctx, x, n_runs, resets, log=False, full_reset=True, T=T):
    """The runs one after the other on input uploaded in place, the marks made in front of their run; per run (records, m17_diag, log)."""
    Cn = x.shape[0]
    if full_reset:
        ctx.reset()
    out = []
    for r in range(n_runs):
        if r in resets:
            ctx.reset_channels(resets[r])
        ctx.upload(x[:, r * T:(r + 1) * T])
        ctx.run()
        out.append((ctx.frames().copy(), ctx.diag(Cn), ctx.diag_log(Cn, capacity=T // 384 + 2) if log else None))
    return out


# the schedule configurations of tests/test_gpu_streaming.py's fixture
@pytest.fixture(scope="module", params=[{}, {15: 0, 17: 0}, {3: 7001}, {3: 9600, 15: 0}, {10: 0, 20: 1, 17: 0}, {26: 1, 3: 4800}, {26: 1, 3: 7001, 15: 0}],
                ids=["default", "decode_and_evm_in_k5", "seg7001", "seg9600_decode_in_k5", "k3_throughput_form_redo_in_front_evm_in_k5", "gate_aware_seg4800", "gate_aware_seg7001_decode_in_k5"])
def ctx(request):
    c = m17hip.Context(64, 48000)
    for k, v in request.param.items():
        c.tune(k, v)
    yield c
    c.close()


@pytest.fixture(params=["fetch_then_run", "run_then_fetch"])
def order(request):
    return request.param


# ---- case 1: the feature is visible ---------------------------------------------------------------------------------------------------
def test_a_reset_channel_is_a_fresh_demodulator_and_that_can_be_seen():
    Cn, n_runs = 12, 3
    x = _stream(Cn, n_runs * T, seed=4101)
    chans = [0, 1, 3, 4, 6, 10]                     # BERT and voice channels: the reset at run 1 falls inside their one transmission
    resets = {1: chans}
    exp = _expect(x, n_runs, resets)
    cont = _expect(x, n_runs, {})                   # the oracle's continuation without the reset
    # the case can fail (a condition on the inputs, checked on the CPU): every reset channel's fresh run yields frames, and they are not the
    # continuation's; at least half of the resets fall inside a locked transmission (the continuation ends run 0 locked: m17_diag.locked)
    for c in chans:
        fresh = np.concatenate([exp[r][0][c] for r in (1, 2)])
        going = np.concatenate([cont[r][0][c] for r in (1, 2)])
        assert fresh.size >= 1 and fresh["seq"][0] == 0 and fresh["sample_pos"][0] < 2 * T, c
        assert fresh.tobytes() != going.tobytes(), c
    assert 2 * sum(int(cont[0][1]["locked"][c]) for c in chans) >= len(chans)
    ctx = m17hip.Context(Cn, T)
    try:
        got = _in_place(ctx, x, n_runs, resets)
    finally:
        ctx.close()
    for r in range(n_runs):
        _assert_run(got[r][0], got[r][1], exp[r], f"run {r}")


def test_resets_at_every_phase_of_the_five_tick_cycle_of_the_carrier_detect_sums():
    """K3 restarts running sum j at the context's ticks = j (mod 5) and a fresh channel's first carrier-detect segment begins at the tick of its reset:
    runs of 126 ticks (24 192 samples) put the resets of a six-run stream at ticks = 1, 2, 3, 4, 0 (mod 5), in place and staged in turn."""
    import torch
    Cn, n_runs, Tn = 24, 6, 126 * 192
    x = _stream(Cn, n_runs * Tn, seed=4801)
    resets = {r: [(5 * r + i) % Cn for i in range(0, 12, 2)] + [r] for r in range(1, n_runs)}
    assert sorted((r * Tn // 192) % 5 for r in resets) == [0, 1, 2, 3, 4]
    exp = _expect(x, n_runs, resets, T=Tn)
    assert all(sum(exp[r][0][c].size for c in resets[r]) > 6 for r in resets)
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * Tn:(r + 1) * Tn])).pin_memory() for r in range(n_runs)]
    c = m17hip.Context(Cn, Tn)
    try:
        c.tune(3, 9600)                                 # (segments inside a run: the replay ahead, the redo and the fold passes take part)
        for r in range(n_runs):
            if r in resets:
                c.reset_channels(resets[r])
            if r % 2:
                c.upload_async(pins[r].data_ptr(), Cn, Tn)
                c.front(channels=Cn, samples=Tn)
                c.run(channels=Cn, samples=Tn)
            else:
                c.upload(x[:, r * Tn:(r + 1) * Tn]); c.run()
            _assert_run(c.frames().copy(), c.diag(Cn), exp[r], f"run {r}")
        c.upload_wait()
    finally:
        c.close()


# ---- case 2: in-place runs ---------------------------------------------------------------------------------------------------------------
_CASE2 = {}


def _case2():
    if not _CASE2:
        Cn, n_runs = 64, 4
        x = _stream(Cn, n_runs * T, seed=4201)
        resets = {1: [0, 1, 2, 5, 15, 16, 17, 31, 33, 40, 47, 63], 3: [1, 3, 4, 8, 16, 32, 48, 62]}   # channels 1 and 16: before both runs
        _CASE2.update(x=x, n_runs=n_runs, resets=resets, exp=_expect(x, n_runs, resets, logs=True))
        reset_recs = sum(_CASE2["exp"][r][0][c].size for r, cs in resets.items() for c in cs)
        assert reset_recs > 40
    return _CASE2


def test_in_place_runs_with_resets_before_two_of_them(ctx):
    k = _case2()
    ctx.tune(9, T // 384 + 2)
    try:
        got = _in_place(ctx, k["x"], k["n_runs"], k["resets"], log=True)
    finally:
        ctx.tune(9, 0)
    for r in range(k["n_runs"]):
        _assert_run(got[r][0], got[r][1], k["exp"][r], f"run {r}", got[r][2])


# ---- case 3: the call orders of a live feed ----------------------------------------------------------------------------------------------
_CASE3 = {}


def _case3():
    if not _CASE3:
        Cn, n_runs = 64, 5
        x = _stream(Cn, n_runs * T, seed=4301)
        resets = {1: [0, 1, 2, 20, 21, 22, 63], 2: [1, 7, 8, 9, 33], 4: [0, 16, 17, 62, 63]}
        _CASE3.update(x=x, n_runs=n_runs, resets=resets, exp=_expect(x, n_runs, resets))
    return _CASE3


def test_live_feed_orders_keep_the_run_before_the_resets_intact(ctx, order):
    """stage(k + 1); reset_channels; front(k + 1); run(k + 1); frames_select(1); fetch(k) — and the older front; fetch(k); run.  Run k's records
    of the reset channels are complete (payload frames whose decode was deferred included: they are decoded after run k + 1 was queued), run
    k + 1's are the fresh ones.  In the older order m17_diag of run k is fetched between front(k + 1) and run(k + 1): still run k's."""
    import torch
    k = _case3()
    x, n_runs, resets, exp = k["x"], k["n_runs"], k["resets"], k["exp"]
    Cn = x.shape[0]
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(n_runs)]
    ctx.reset()
    ctx.upload_async(pins[0].data_ptr(), Cn, T)
    ctx.run(channels=Cn, samples=T)
    for r in range(n_runs):
        d = None
        if r + 1 < n_runs:
            ctx.upload_async(pins[r + 1].data_ptr(), Cn, T)
            if r + 1 in resets:
                ctx.reset_channels(resets[r + 1])
            ctx.front(channels=Cn, samples=T)
            if order == "run_then_fetch":
                ctx.run(channels=Cn, samples=T)
                ctx.frames_select(1)
            else:
                d = ctx.diag(Cn)
        got = ctx.frames().copy()
        ctx.frames_select(0)
        if r + 1 < n_runs and order != "run_then_fetch":
            ctx.run(channels=Cn, samples=T)
        if r + 1 == n_runs:
            d = ctx.diag(Cn)
        _assert_run(got, d, exp[r], f"{order}, run {r}")
    ctx.upload_wait()


def test_staged_runs_without_a_front_call_and_in_place_runs_mixed(ctx):
    """The same stream with the run call itself beginning the staged runs (no m17hip_demod_front), and every other run uploaded in place."""
    import torch
    k = _case3()
    x, n_runs, resets, exp = k["x"], k["n_runs"], k["resets"], k["exp"]
    Cn = x.shape[0]
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(n_runs)]
    ctx.reset()
    for r in range(n_runs):
        if r in resets:
            ctx.reset_channels(resets[r][: len(resets[r]) // 2])
            ctx.reset_channels(resets[r][len(resets[r]) // 2 - 1:])        # several calls before one run add up; duplicates are allowed
        if r % 3 == 2:
            ctx.upload(x[:, r * T:(r + 1) * T])
            ctx.run()
        else:
            ctx.upload_async(pins[r].data_ptr(), Cn, T)
            ctx.run(channels=Cn, samples=T)
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[r], f"run {r}")
    ctx.upload_wait()


def test_the_cxx_wrapper_resets_the_listed_channels(tmp_path):
    """BatchedDemodulator::reset_channels from a C++ host (tests/cxx/reset_channels_check.cpp): run, reset three channels, run."""
    import subprocess
    from test_channel_reset_args import build_cxx_driver
    Cn, chans = 9, [0, 4, 7]
    x = _stream(Cn, 2 * T, seed=4901)
    exp = _expect(x, 2, {1: chans})
    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "x.i16", tmp_path / "out.recs"
    x.tofile(src)
    r = subprocess.run([exe, str(src), str(Cn), str(T), str(dst)] + [str(c) for c in chans], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n0, n1 = (int(v) for v in r.stdout.split())
    got = np.fromfile(dst, dtype=m17hip.FRAME_REC)
    assert got.size == n0 + n1
    _assert_run(got[:n0], None, exp[0], "run 0")
    _assert_run(got[n0:], None, exp[1], "run 1")
    assert all(exp[1][0][c].size and exp[1][0][c]["seq"][0] == 0 for c in (0, 4))


# ---- case 4: every channel through the list == m17hip_demod_reset --------------------------------------------------------------------------
def test_resetting_every_channel_through_the_list_equals_a_full_reset():
    Cn, n_runs = 48, 3
    x = _stream(Cn, n_runs * T, seed=4401)
    out = []
    for how in ("list", "full"):
        c = m17hip.Context(Cn, T)
        try:
            c.tune(6, 1); c.tune(7, 64)
            c.upload(x[:, :T]); c.run(); c.frames()
            if how == "list":
                c.reset_channels(np.arange(Cn)[::-1])
            else:
                c.reset()
            res = []
            for r in (1, 2):
                c.upload(x[:, r * T:(r + 1) * T]); c.run()
                res.append((c.frames().tobytes(), c.diag(Cn).tobytes(), c.bert_stats(Cn).tobytes(), c.packets().tobytes()))
            out.append(res)
        finally:
            c.close()
    assert len(out[0][0][0]) > 64 * Cn
    for r in range(2):
        for i, what in enumerate(("records", "m17_diag", "BERT statistics", "packets")):
            assert out[0][r][i] == out[1][r][i], (r, what)


# ---- case 5: the payload consumers -------------------------------------------------------------------------------------------------------
def _assemble(asm, recs):
    out = asm.feed(recs["frame_type"], recs["payload"]) if recs.size else []
    for e in out:
        e["pos"] = int(recs[e["rec_index"]]["sample_pos"])
    return out


def test_consumers_of_a_reset_channel_start_over(order):
    """BERT statistics of a reset channel == the PRBS9 receiver over its post-reset records alone; a packet channel reset in the middle of a packet
    completes no packet from the abandoned frames and numbers its packets from zero again — against the CPU consumers of the parity tests, in
    both call orders of a live feed (the consumers of run k work after run k + 1, which resets them, was queued)."""
    import torch
    Cn, n_runs = 24, 5
    x = _stream(Cn, n_runs * T, seed=4501)
    # runs 1 and 3 begin inside a packet (its frames run up to sample 39 500 of its 48 000), runs 2 and 4 between two
    resets = {1: [0, 2, 5, 9], 2: [1, 8, 11, 14], 3: [3, 5, 17, 23], 4: [6, 14, 20]}
    exp = _expect(x, n_runs, resets)
    org = _origins(Cn, n_runs, resets)
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(n_runs)]
    c = m17hip.Context(Cn, T)
    try:
        c.tune(6, 1); c.tune(7, 64)
        c.reset()
        c.upload_async(pins[0].data_ptr(), Cn, T)
        c.run(channels=Cn, samples=T)
        pk = []
        for r in range(n_runs):
            if r + 1 < n_runs:
                c.upload_async(pins[r + 1].data_ptr(), Cn, T)
                if r + 1 in resets:
                    c.reset_channels(resets[r + 1])
                c.front(channels=Cn, samples=T)
                if order == "run_then_fetch":
                    c.run(channels=Cn, samples=T)
                    c.frames_select(1)
            _assert_run(c.frames().copy(), None, exp[r], f"{order}, run {r}")
            pk.append(c.packets().copy())
            c.frames_select(0)
            if r + 1 < n_runs and order != "run_then_fetch":
                c.run(channels=Cn, samples=T)
        c.upload_wait()
        st = c.bert_stats(Cn)
    finally:
        c.close()
    n_packets = 0
    for ch in range(Cn):
        a = int(org[n_runs - 1][ch])                                   # the channel's latest reset: the statistics are of the records since
        since = np.concatenate([exp[r][0][ch] for r in range(a, n_runs)])
        bert = since[since["frame_type"] == 5]
        bits, errs, sync = ol.bert_count(bert["payload"][:, :25]) if bert.size else (0, 0, False)
        assert (int(st["bits"][ch]), int(st["errors"][ch]), bool(st["synced"][ch]), int(st["frames"][ch])) == (bits, errs, sync, bert.size), ch
        asm, seq = ol.PacketAssembler(), 0
        for r in range(n_runs):
            if r and org[r][ch] != org[r - 1][ch]:
                asm, seq = ol.PacketAssembler(), 0                     # (a fresh consumer with the fresh demodulator)
            want = _assemble(asm, exp[r][0][ch])
            got = pk[r][pk[r]["channel"] == ch]
            assert got.size == len(want), (ch, r, got.size, len(want))
            for g, w in zip(got, want):
                assert (int(g["seq"]), int(g["sample_pos"]), int(g["size"]), int(g["checksum"]), int(g["frames"]), int(g["seq_errors"])) == \
                       (seq, w["pos"], w["size"], w["checksum"], w["frames"], w["seq_errors"]), (ch, r)
                assert g["data"].tobytes() == w["data"].tobytes() and int(g["crc_ok"]) == int(w["checksum"] == 0x0F47), (ch, r)
                seq += 1
                n_packets += 1
    assert n_packets >= Cn // 4
    # reset inside their first packet (run 1): nothing is completed from its frames, neither the abandoned nor the headless ones
    for ch in (2, 5):
        assert not any((p["channel"] == ch).any() for p in pk[:2]), ch
    # reset between two packets (run 2), after the first was completed: the second one is this demodulator's packet 0 again
    for ch in (8, 11, 14):
        first, again = pk[1][pk[1]["channel"] == ch], pk[3][pk[3]["channel"] == ch]
        assert first.size == 1 and again.size == 1 and int(first["seq"][0]) == 0 and int(again["seq"][0]) == 0, ch
        assert 0 < int(again["sample_pos"][0]) < 2 * T, ch
    assert int((st["frames"] > 0).sum()) >= Cn // 3


# ---- case 6: size ------------------------------------------------------------------------------------------------------------------------
def test_4096_channels_a_quarter_of_them_reset_at_each_boundary():
    Cn, n_runs = 4096, 3
    p = ol.gen_params(seed=4601, kind=-1, n_frames=n_runs * T // 1920 - 4, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0,
                      total=n_runs * T)
    x = ol.generate_batch(p, Cn, n_runs * T, threads=THREADS)
    rng = np.random.default_rng(4602)
    resets = {}
    for r in (1, 2):    # scattered indices, the first and the last channel included, within and across the 16-channel groups of K2 and the fold pass
        pick = set(rng.choice(Cn, size=Cn // 4, replace=False).tolist()) | {0, Cn - 1, 15, 16, 17, 31, 32}
        resets[r] = sorted(pick)
    exp = _expect(x, n_runs, resets)
    ctx = m17hip.Context(Cn, T)
    try:
        got = _in_place(ctx, x, n_runs, resets)
    finally:
        ctx.close()
    for r in range(n_runs):
        _assert_run(got[r][0], got[r][1], exp[r], f"run {r}")
    assert sum(exp[2][0][c].size for c in resets[2]) > Cn // 8


# ---- case 7: refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_mark_nothing():
    import torch
    Cn = 8
    x = _stream(Cn, 3 * T, seed=4701)
    whole = _expect(x, 3, {})
    c = m17hip.Context(Cn, T)
    lib, h = c.lib, c.h

    def call(idx):
        a = np.asarray(idx, dtype=np.uint32)
        return lib.m17hip_demod_reset_channels(h, a.ctypes.data_as(C.c_void_p) if a.size else None, C.c_uint32(a.size))

    try:
        assert call([]) == 0                                            # n == 0: a successful no-op
        assert call([1, 1, 3]) == 0                                     # before the first run after a full reset: nothing observable
        assert call([0, Cn]) == EINVAL                                  # out of range: nothing is marked, channel 0 included
        assert lib.m17hip_demod_reset_channels(h, None, C.c_uint32(2)) == EINVAL
        c.upload(x[:, :T]); c.run()
        _assert_run(c.frames().copy(), c.diag(Cn), whole[0], "after the refusals of arguments")
        pin = torch.from_numpy(np.ascontiguousarray(x[:, T:2 * T])).pin_memory()
        c.upload_async(pin.data_ptr(), Cn, T)
        c.front(channels=Cn, samples=T)
        assert call([2]) == ESTATE                                      # between front and run
        c.run(channels=Cn, samples=T)
        c.upload_wait()
        _assert_run(c.frames().copy(), c.diag(Cn), whole[1], "after the refusal between front and run")
        c.upload(x[:, 2 * T:]); c.run()
        _assert_run(c.frames().copy(), c.diag(Cn), whole[2], "the run after it")
        # a first run of 1000 samples: the position is not a multiple of 192
        c.reset()
        c.upload(x[:, :1000]); c.run()
        assert call([0, 1]) == ESTATE
        c.upload(x[:, 1000:T + 1000]); c.run()
        recs, counts, d = ol.demod_batch(np.ascontiguousarray(x[:, :T + 1000]), cap=64, threads=THREADS)
        e = np.concatenate([recs[i, : counts[i]][recs[i, : counts[i]]["sample_pos"] >= 1000] for i in range(Cn)])
        assert c.frames().tobytes() == e.tobytes() and e.size > Cn
        g = c.diag(Cn)
        for f in INT_FIELDS + FLOAT_FIELDS:
            assert np.array_equal(g[f], d[f], equal_nan=True), f
    finally:
        c.close()
