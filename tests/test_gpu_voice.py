"""GPU: the voice consumer (m17hip_tune key 34; csrc/m17_voice_kernel.hpp) — codec2 payload planes, mark bytes and the per-channel call log —
against the plain-Python restatement of its rules (tests/voice_log.py): on hand-made records through m17hip_voice_feed, where every branch is
placed exactly, and end to end on transmissions of the test's own content (m17hip_synth_tx_i16), where the oracle supplies the records the
restatement is run over.  Byte for byte: planes, marks, counts, calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import tx_build as tb
import voice_log as vl

pytestmark = pytest.mark.gpu

MAXC, MAXT = 70, 192000
OK, EINVAL, ESTATE, EOVERFLOW, ETRUNC = 0, -1, -4, -5, -6
PITCH = 150


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(MAXC, MAXT)
    yield c
    c.close()


# ---- the C calls with their return codes (the Python wrappers raise on M17HIP_EOVERFLOW / M17HIP_ETRUNC) ---------------------------------------
def raw_voice(ctx, channels, slots):
    audio = np.full((channels, slots, 16), 0xEE, dtype=np.uint8)
    marks = np.full((channels, slots), 0xEE, dtype=np.uint8)
    counts = np.zeros(channels, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    code = ctx.lib.m17hip_voice_fetch(ctx.h, p(audio), p(marks), p(counts), C.c_uint32(channels), C.c_uint32(slots))
    return code, audio, marks, counts


def raw_calls(ctx, capacity):
    out = np.zeros(capacity, dtype=m17hip.CALL_REC)
    n = C.c_uint32(0)
    code = ctx.lib.m17hip_calls_fetch(ctx.h, out.ctypes.data_as(C.c_void_p) if capacity else None, C.c_uint32(capacity), C.byref(n))
    return code, out[:min(n.value, capacity)], n.value


def assert_planes(got, exp, what=""):
    """(audio, marks, counts[, calls]) of the library against the restatement's: the slots in use byte for byte, the calls byte for byte."""
    assert np.array_equal(got[2], exp[2]), (what, got[2].tolist(), exp[2].tolist())
    for c, n in enumerate(exp[2]):
        assert np.array_equal(got[1][c, :n], exp[1][c, :n]), (what, c, got[1][c, :n].tolist(), exp[1][c, :n].tolist())
        assert np.array_equal(got[0][c, :n], exp[0][c, :n]), (what, c)
    if len(exp) > 3:
        assert got[3].size == exp[3].size, (what, got[3].tolist(), exp[3].tolist())
        assert got[3].tobytes() == exp[3].tobytes(), (what, [i for i in range(exp[3].size) if got[3][i] != exp[3][i]][:4])


def fetched(ctx, channels, slots=None):
    audio, marks, counts = ctx.voice(slots=slots, channels=channels)
    return audio, marks, counts, ctx.calls(capacity=channels * m17hip.calls_per_channel(PITCH))


# ---- 1. feed: every branch, placed by hand ---------------------------------------------------------------------------------------------------------
def rec(ftype, pos, cost=0, payload=b""):
    r = np.zeros((), dtype=m17hip.FRAME_REC)
    r["frame_type"], r["sample_pos"], r["cost"], r["len"] = ftype, pos, cost, len(payload)
    r["payload"] = np.frombuffer(bytes(payload).ljust(32, b"\xa5"), dtype=np.uint8)   # (what lies behind a payload is not the consumer's)
    return r


class Maker:
    """Hand-made records of one channel: positions go up, frame numbers go on from batch to batch."""

    def __init__(self, seed, pos=0, fn=0):
        self.rng, self.pos, self.fn = np.random.default_rng(seed), pos, fn

    def step(self):
        self.pos += 1920
        return self.pos

    def lsf(self):
        return rec(vl.FT_LSF, self.step(), int(self.rng.integers(0, 40)), bytes(self.rng.integers(0, 256, 30, dtype=np.uint8)))

    def voice(self, cost=None, eos=False, jump=0):
        self.fn = (self.fn + jump) & 0x7FFF
        cost = int(self.rng.choice([0, 3, 69, 70, 80, 81, 150])) if cost is None else cost
        r = rec(vl.FT_STREAM, self.step(), cost, m17hip.stream_row(self.fn, self.rng.integers(0, 256, 16, dtype=np.uint8), last=eos)[:18])
        self.fn = (self.fn + 1) & 0x7FFF
        return r

    def other(self):
        t = int(self.rng.choice([1, 3, 4, 5]))
        return rec(t, self.step(), int(self.rng.integers(0, 200)), bytes(self.rng.integers(0, 256, {1: 6, 3: 26, 4: 26, 5: 25}[t], dtype=np.uint8)))

    def random(self, n):
        out = []
        for _ in range(n):
            u = self.rng.random()
            if u < 0.04:
                out.append(self.lsf())
            elif u < 0.24:
                out.append(self.other())
            else:
                out.append(self.voice(eos=self.rng.random() < 0.06, jump=int(self.rng.integers(1, 5)) if self.rng.random() < 0.1 else 0))
        return out

    def plain(self, n):
        return [self.voice(cost=5) for _ in range(n)]


def feed_batches():
    """Two batches of 70 rows (lists of records).  The pass boundary (record 64 of a row) falls inside a call (5), on an LSF (6, 9), behind and on an
    accepted EOS (7, 8); counts of 0, 1, 63, 64, 65 and 150; frame numbers that wrap (every fifth channel); positions beyond 2^32 (13)."""
    makers = [Maker(1000 + c, pos=(1 << 33) + 5 if c == 13 else 100 * c, fn=0x7FF0 if c % 5 == 0 else 3 * c) for c in range(MAXC)]
    counts = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 10: 1, 11: 1, 12: 2, 14: 128, 15: 129, 16: 150, 17: 150}
    b1, b2 = [], []
    for c, m in enumerate(makers):
        if c == 5:
            rows = [m.lsf()] + m.plain(149)                                  # one call open over the whole batch ...
        elif c == 6:
            rows = m.plain(64) + [m.lsf()] + m.plain(85)
        elif c == 7:
            rows = [m.lsf()] + m.plain(62) + [m.voice(cost=69, eos=True)] + m.plain(86)
        elif c == 8:
            rows = [m.lsf()] + m.plain(63) + [m.voice(cost=0, eos=True)] + [m.other()] + m.plain(84)
        elif c == 9:
            rows = m.plain(63) + [m.lsf()] + m.plain(63) + [m.voice(cost=10, eos=True), m.voice(cost=10, eos=True)] + m.plain(21)
        elif c == 10:
            rows = [m.lsf()]
        elif c == 11:
            rows = [m.voice(cost=1, eos=True)]
        else:
            rows = m.random(counts.get(c, int(m.rng.integers(0, PITCH + 1))))
        b1.append(rows)
    for c, m in enumerate(makers):
        if c == 5:
            rows = m.plain(10) + [m.voice(cost=7, eos=True)] + m.random(60)  # ... and closed by the second
        elif c in (10, 11):
            rows = m.plain(3)
        elif c == 2:
            rows = []
        else:
            rows = m.random(int(m.rng.integers(0, PITCH + 1)))
        b2.append(rows)
    return b1, b2


def packed(rows):
    """[70][PITCH] records and counts; what lies behind a row's count is filled with records that would change everything if they were read."""
    trap = rec(vl.FT_STREAM, 7, 0, m17hip.stream_row(0x1234, b"\xee" * 16, last=True)[:18])
    recs = np.zeros((len(rows), PITCH), dtype=m17hip.FRAME_REC)
    recs[:] = trap
    for c, r in enumerate(rows):
        for i, q in enumerate(r):
            recs[c, i] = q
            recs[c, i]["channel"], recs[c, i]["seq"] = c, i
    return recs, np.array([len(r) for r in rows], dtype=np.uint32)


def test_feed_every_branch_and_state_carried_between_batches(ctx):
    b1, b2 = feed_batches()
    assert sorted(set(len(r) for r in b1) & {0, 1, 63, 64, 65, 150}) == [0, 1, 63, 64, 65, 150]
    assert b1[6][64]["frame_type"] == vl.FT_LSF and b1[7][63]["payload"][0] & 0x80 and b1[8][64]["payload"][0] & 0x80 and b1[9][63]["frame_type"] == vl.FT_LSF
    bank = vl.VoiceBank(MAXC, channel_base=500)
    ctx.set_channel_base(500)
    ctx.tune(34, PITCH)
    try:
        ctx.reset()
        assert raw_voice(ctx, MAXC, 4)[0] == ESTATE and raw_calls(ctx, 4)[0] == ESTATE       # nothing run, nothing fed
        first = None
        for k, rows in enumerate((b1, b2)):
            exp = bank.feed(rows)
            assert max(np.bincount(exp[3]["channel"] - 500, minlength=MAXC)) <= m17hip.calls_per_channel(PITCH)   # (the room is not what is tested here)
            ctx.voice_feed(*packed(rows))
            got = fetched(ctx, MAXC)
            assert_planes(got, exp, f"batch {k}")
            marks = np.concatenate([exp[1][c, :n] for c, n in enumerate(exp[2])])
            assert all((marks & bit).any() for bit in (1, 2, 4, 8)) and (exp[3]["close"] == 1).any() and (exp[3]["close"] == 2).any()
            assert (exp[3]["has_lsf"] == 0).any() and (exp[3]["lost"] > 0).any() and (exp[3]["blanked"] > 0).any()
            first = first or exp
        # channel 5's call: opened by batch 1's first record, closed by batch 2's eleventh voice frame, reported once with everything it saw
        mine = got[3][got[3]["channel"] == 505]
        assert first[3][first[3]["channel"] == 505].size == 0 and mine.size >= 1
        c5 = mine[0]
        assert (int(c5["seq"]), int(c5["start_pos"]), int(c5["frames"]), int(c5["cost_sum"]), int(c5["close"])) == \
            (0, int(b1[5][0]["sample_pos"]), 149 + 11, 149 * 5 + 10 * 5 + 7, 1)
        assert int(c5["end_pos"]) == int(b2[5][10]["sample_pos"]) and bytes(c5["lsf"]) == bytes(b1[5][0]["payload"][:30])
        # rows cut at `slots`: the same bytes, narrower
        code, audio, marks, counts = raw_voice(ctx, MAXC, 40)
        assert code == ETRUNC and np.array_equal(counts, exp[2])
        for c, n in enumerate(exp[2]):
            n = min(int(n), 40)
            assert np.array_equal(audio[c, :n], exp[0][c, :n]) and np.array_equal(marks[c, :n], exp[1][c, :n]), c
        # the device pointers name the same planes: viewed as torch tensors where they lie
        import torch
        a_dev, m_dev, n_dev, pitch = ctx.voice_device()
        assert a_dev and m_dev and n_dev and pitch == PITCH
        view = lambda ptr, shape, typestr: torch.as_tensor(type("DeviceView", (), {"__cuda_array_interface__": dict(
            shape=shape, typestr=typestr, data=(ptr, False), version=2)})(), device="cuda")
        assert np.array_equal(view(n_dev, (MAXC,), "<i4").cpu().numpy().astype(np.uint32), exp[2])
        a_t, m_t = view(a_dev, (MAXC, PITCH, 16), "|u1").cpu().numpy(), view(m_dev, (MAXC, PITCH), "|u1").cpu().numpy()
        assert_planes((a_t, m_t, exp[2]), exp[:3], "device view")
        # a reset starts every channel over
        ctx.reset()
        fresh = vl.VoiceBank(MAXC, channel_base=500)
        ctx.voice_feed(*packed(b2))
        assert_planes(fetched(ctx, MAXC), fresh.feed(b2), "after reset")
    finally:
        ctx.tune(34, 0)
        ctx.set_channel_base(0)
        ctx.reset()


def test_feed_more_calls_than_the_room(ctx):
    """Room 8: M17HIP_CALLS_PER_CHANNEL(8) = 3 calls per channel and run.  A channel that closes nine keeps its first three (M17HIP_EOVERFLOW); the
    channels beside it are whole, and so is its own state (seq goes on counting)."""
    room = m17hip.calls_per_channel(8)
    makers = [Maker(70 + c) for c in range(3)]
    rows = [[makers[0].lsf() for _ in range(10)], [makers[1].voice(cost=0, eos=True) for _ in range(room)], [makers[2].lsf(), makers[2].lsf()]]
    exp = vl.VoiceBank(3).feed(rows)
    ctx.tune(34, 8)
    try:
        ctx.reset()
        recs, counts = packed(rows)
        ctx.voice_feed(recs[:, :16].copy(), counts)
        code, calls, n = raw_calls(ctx, 64)
        assert code == EOVERFLOW and n == 9 + room + 1
        keep = np.concatenate([exp[3][exp[3]["channel"] == 0][:room], exp[3][exp[3]["channel"] != 0]])
        assert calls[:keep.size].tobytes() == keep.tobytes() and not calls[keep.size:].tobytes().strip(b"\0")   # (*count: how many there were)
        code, calls, n = raw_calls(ctx, 2)                                   # the truncation rule of m17hip_packets_fetch
        assert n == 9 + room + 1 and calls.tobytes() == keep[:2].tobytes()
        ctx.voice_feed(recs[:1, :2].copy(), counts[:1] * 0 + 2)              # two more LSFs: calls 9 and 10 of channel 0
        code, calls, n = raw_calls(ctx, 64)
        assert code == OK and calls["seq"].tolist() == [9, 10]
    finally:
        ctx.tune(34, 0)
        ctx.reset()


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------------------------
E2E_C, E2E_T = 5, 192000
_E2E = {}


def transmissions():
    rng = np.random.default_rng(6061)
    pay = lambda: rng.integers(0, 256, 16, dtype=np.uint8)
    lsfs = [m17hip.make_lsf("", "N0CALL", 0x0005), m17hip.make_lsf("W1AW/P", "SP5WWP-9", 0x0005, b"voice"), m17hip.make_lsf("AB1CDE", "K-./", 0x0005)]
    skipping = [f for f in range(23) if not 7 <= f <= 9]
    return [(tb.STREAM, lsfs[0], [m17hip.stream_row(i, pay(), last=i == 69) for i in range(70)]),
            (tb.STREAM, lsfs[1], [m17hip.stream_row(i, pay(), last=i == 11) for i in range(12)]),
            (tb.STREAM, lsfs[2], [m17hip.stream_row(f, pay(), last=f == 22) for f in skipping]),
            (tb.BERT, None, [bytes(rng.integers(0, 256, 24, dtype=np.uint8)) + bytes([int(rng.integers(0, 32)) << 3]) for _ in range(30)]),
            (tb.PACKET, m17hip.make_lsf("", "N0CALL", 0x0002),
             [bytes(rng.integers(0, 256, 25, dtype=np.uint8)) + bytes([0x80 | 25 << 2 if i == 4 else i << 2]) for i in range(5)])]


def e2e(ctx):
    """The input (synthesised on the device, read back), the oracle's records of it and what the restatement makes of them: once per session.
    (seed 1, sigma 600: the noise of tests/test_gpu_synth_tx.py; with it the oracle acquires all five transmissions.)"""
    if not _E2E:
        base = ol.gen_params(seed=1, lead_in=3072, lead_sigma=40000.0, noise_sigma=600.0, tail_sigma=600.0)
        ctx.synth_tx(base, transmissions(), E2E_T)
        x = ctx.download()
        recs, counts, _ = ol.demod_batch(x, cap=2 * (E2E_T // 1920 + 2) + 4, threads=E2E_C)
        rows = [recs[c, :counts[c]] for c in range(E2E_C)]
        exp = vl.VoiceBank(E2E_C).feed(rows)
        # what makes the case bite, on the oracle's records alone
        assert exp[2][0] > 64 and exp[2][3] == 0 and exp[2][4] == 0 and (rows[3]["frame_type"] == 5).sum() >= 20 and (rows[4]["frame_type"] == 3).sum() == 5
        by = {int(c["channel"]): c for c in exp[3]}
        assert by[0]["frames"] == 70 and by[1]["close"] == vl.CLOSE_EOS and by[1]["frames"] == 12 and by[2]["lost"] == 3 and by[2]["frames"] == 20
        assert all(bytes(by[c]["lsf"]) == transmissions()[c][1] for c in range(3))
        _E2E.update(x=x, rows=rows, exp=exp, flat=np.concatenate(rows))
    return _E2E


@pytest.mark.parametrize("defer", [1, 0])
def test_end_to_end_against_the_oracles_records(ctx, defer):
    """Key 15 at its default — the stream payloads are only there after decode_deferred_kernel, which the consumer must run behind — and at 0."""
    d = e2e(ctx)
    ctx.tune(34, PITCH)
    ctx.tune(15, defer)
    try:
        ctx.upload(d["x"]); ctx.reset(); ctx.run()
        got = fetched(ctx, E2E_C)
        assert ctx.frames().tobytes() == d["flat"].tobytes()
        assert_planes(got, d["exp"], f"key 15 = {defer}")
    finally:
        ctx.tune(15, 1)
        ctx.tune(34, 0)


def test_cxx_wrapper_end_to_end(ctx, tmp_path):
    """BatchedDemodulator::enable_voice / voice / calls (tests/cxx/voice_check.cpp) print what the restatement says."""
    import test_voice_log as tv
    d = e2e(ctx)
    exe = tv.build_cxx_driver(tmp_path)
    d["x"].tofile(tmp_path / "x.i16")
    r = subprocess.run([exe, str(tmp_path / "x.i16"), str(E2E_C), str(E2E_T), str(PITCH)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    audio, marks, counts, calls = d["exp"]
    for c in range(E2E_C):
        n = int(counts[c])
        want = f"{c} {n} " + (bytes(marks[c, :n]).hex() + " " + bytes(audio[c, 0]).hex() if n else "- -")
        assert lines[c] == want, c
    want = ["call " + " ".join(str(int(q[f])) for f in ("channel", "seq", "start_pos", "end_pos", "frames", "blanked", "lost", "cost_sum", "has_lsf", "close"))
            for q in calls]
    assert lines[E2E_C:] == want


# ---- 3. across runs and fetch orders ---------------------------------------------------------------------------------------------------------------
def collect(parts, got):
    parts.append(got)


def joined(parts, channels):
    """The runs' planes one behind the other per channel, and the union of their calls in (channel, seq) order."""
    counts = np.sum([p[2] for p in parts], axis=0).astype(np.uint32)
    n = int(counts.max())
    audio, marks = np.zeros((channels, n, 16), dtype=np.uint8), np.zeros((channels, n), dtype=np.uint8)
    for c in range(channels):
        at = 0
        for a, m, k, _ in parts:
            audio[c, at:at + k[c]], marks[c, at:at + k[c]] = a[c, :k[c]], m[c, :k[c]]
            at += int(k[c])
    calls = np.concatenate([p[3] for p in parts])
    return audio, marks, counts, calls[np.lexsort((calls["seq"], calls["channel"]))]


def chunked(ctx, x, lengths, staged):
    """The stream in runs of the given lengths.  Staged: stage(k + 1); front; run(k + 1); frames_select(1); fetch run k — the live feed's order."""
    parts, lo = [], 0
    ctx.reset()
    for k, L in enumerate(lengths):
        chunk = np.ascontiguousarray(x[:, lo:lo + L])
        lo += L
        if not staged or k == 0:
            ctx.upload(chunk); ctx.run()
            if not staged:
                collect(parts, fetched(ctx, x.shape[0]))
            continue
        ctx.tune(16, 1); ctx.upload(chunk); ctx.tune(16, 0)
        ctx.front(); ctx.run()
        ctx.frames_select(1)
        collect(parts, fetched(ctx, x.shape[0]))
        ctx.frames_select(0)
    if staged:
        collect(parts, fetched(ctx, x.shape[0]))
    return parts


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("length", [48000, 1927])
def test_runs_of_a_stream_report_each_call_once(ctx, length, staged):
    d = e2e(ctx)
    lengths = [length] * (E2E_T // length) + ([E2E_T % length] if E2E_T % length else [])
    ctx.tune(34, PITCH)
    try:
        parts = chunked(ctx, d["x"], lengths, staged)
    finally:
        ctx.tune(34, 0)
    assert_planes(joined(parts, E2E_C), d["exp"], f"runs of {length}, staged {staged}")
    # a call that spans run boundaries is reported by the run that closes it, and by no other
    ends = np.cumsum(lengths)
    run_of = lambda pos: int(np.searchsorted(ends, int(pos), side="right"))
    assert (d["exp"][3]["close"] == vl.CLOSE_EOS).all()                      # (so the closing record is the one at end_pos)
    assert any(run_of(q["start_pos"]) < run_of(q["end_pos"]) for q in d["exp"][3])
    for q in d["exp"][3]:
        k = run_of(q["end_pos"])
        where = [i for i, p in enumerate(parts) if ((p[3]["channel"] == q["channel"]) & (p[3]["seq"] == q["seq"])).any()]
        assert where == [k], (int(q["channel"]), where, k)


# ---- 4. resets -------------------------------------------------------------------------------------------------------------------------------------
def test_a_channel_reset_abandons_its_open_call(ctx):
    """The stream up to the cut, channel 1 reset, the rest of it — then one hand-made LSF record per channel through m17hip_voice_feed, which
    closes whatever each channel has open and so shows every channel's seq (behind its EOT a continued demodulator yields no further LSF on
    this input, searched on the CPU: without the fed record channel 1 would close nothing after its reset)."""
    d = e2e(ctx)
    cut = 9600                                                               # a multiple of 192 inside channel 1's call
    c1 = d["exp"][3][d["exp"][3]["channel"] == 1][0]
    assert cut % 192 == 0 and int(c1["start_pos"]) < cut < int(c1["end_pos"])
    closing = [[rec(vl.FT_LSF, 10 ** 6 + c, 0, bytes([c]) * 30)] for c in range(E2E_C)]
    twin = m17hip.Context(E2E_C, E2E_T)
    try:
        got, undisturbed = [], []
        for c, parts in ((ctx, got), (twin, undisturbed)):
            c.tune(34, PITCH)
            c.reset()
            c.upload(np.ascontiguousarray(d["x"][:, :cut])); c.run()
            parts.append(fetched(c, E2E_C))
            if c is ctx:
                c.reset_channels([1])
            c.upload(np.ascontiguousarray(d["x"][:, cut:])); c.run()
            parts.append(fetched(c, E2E_C))
            c.voice_feed(*packed(closing))
            parts.append(fetched(c, E2E_C))
    finally:
        twin.close()
        ctx.tune(34, 0)
    bank = vl.VoiceBank(E2E_C)
    assert_planes(joined(undisturbed[:2], E2E_C), bank.feed(d["rows"]), "twin")
    assert_planes(undisturbed[2], bank.feed(closing), "twin, closing records")
    # channel 1 after the reset: a reference process started at the cut, and a consumer that knows nothing of what came before
    recs, _ = ol.demod(d["x"][1, cut:], cap=2 * (E2E_T // 1920 + 2) + 4)
    log = vl.VoiceLog(1)
    a1, m1, calls1 = log.feed(recs)
    assert m1.size >= 1 and calls1.size == 0 and log.call is not None        # (it has a call open at the end, and has closed none)
    _, _, closed1 = log.feed(closing[1])
    assert closed1.size == 1 and closed1[0]["seq"] == 0 and closed1[0]["frames"] == m1.size
    assert not (got[0][3]["channel"] == 1).any() and not (got[1][3]["channel"] == 1).any()   # the abandoned call is never reported
    assert int(got[1][2][1]) == m1.size and np.array_equal(got[1][1][1, :m1.size], m1) and np.array_equal(got[1][0][1, :m1.size], a1)
    mine = got[2][3][got[2][3]["channel"] == 1]
    assert mine.tobytes() == closed1.tobytes()
    theirs = undisturbed[2][3][undisturbed[2][3]["channel"] == 1]
    assert theirs["seq"].tolist() == [1] and int(theirs[0]["start_pos"]) > int(c1["end_pos"])   # (the twin had reported channel 1's call as seq 0)
    # the others: what the twin saw, run by run
    for k in range(3):
        for c in (0, 2, 3, 4):
            n = int(undisturbed[k][2][c])
            assert int(got[k][2][c]) == n and np.array_equal(got[k][0][c, :n], undisturbed[k][0][c, :n]) and np.array_equal(got[k][1][c, :n], undisturbed[k][1][c, :n])
        keep = lambda calls: calls[calls["channel"] != 1].tobytes()
        assert keep(got[k][3]) == keep(undisturbed[k][3])


# ---- 5. limits and the off-switch --------------------------------------------------------------------------------------------------------------------
def test_more_voice_records_than_the_room(ctx):
    d = e2e(ctx)
    audio, marks, counts, calls = d["exp"]
    ctx.tune(34, 8)
    try:
        ctx.upload(d["x"]); ctx.reset(); ctx.run()
        code, a, m, n = raw_voice(ctx, E2E_C, 8)
        assert code == EOVERFLOW and np.array_equal(n, counts)               # counts say how many there were
        for c in range(E2E_C):
            k = min(int(counts[c]), 8)
            assert np.array_equal(a[c, :k], audio[c, :k]) and np.array_equal(m[c, :k], marks[c, :k]), c
        code, got, total = raw_calls(ctx, 64)                                # the accounting went on over every record
        assert code == OK and total == calls.size and got.tobytes() == calls.tobytes()
        code, a, m, n = raw_voice(ctx, E2E_C, 20)                            # slots beyond the room are not written
        assert code == EOVERFLOW and (a[:, 8:] == 0xEE).all() and (m[:, 8:] == 0xEE).all() and np.array_equal(a[0, :8], audio[0, :8])
    finally:
        ctx.tune(34, 0)


def test_fewer_slots_than_records_and_the_switch_off(ctx):
    d = e2e(ctx)
    audio, marks, counts, calls = d["exp"]
    ctx.tune(34, PITCH)
    try:
        ctx.upload(d["x"]); ctx.reset(); ctx.run()
        on = ctx.frames().copy()
        code, a, m, n = raw_voice(ctx, E2E_C, 10)
        assert code == ETRUNC and np.array_equal(n, counts)
        for c in range(E2E_C):
            k = min(int(counts[c]), 10)
            assert np.array_equal(a[c, :k], audio[c, :k]) and np.array_equal(m[c, :k], marks[c, :k]), c
        assert raw_voice(ctx, E2E_C, int(counts.max()))[0] == OK
        assert raw_voice(ctx, 0, 4)[0] == EINVAL and raw_voice(ctx, MAXC, 4)[0] == EINVAL   # no channels; more than the run had
        assert ctx.lib.m17hip_voice_fetch(ctx.h, None, None, None, C.c_uint32(E2E_C), C.c_uint32(0)) == EINVAL
        n32 = C.c_uint32(0)
        assert ctx.lib.m17hip_calls_fetch(ctx.h, None, C.c_uint32(4), C.byref(n32)) == EINVAL
        assert ctx.lib.m17hip_voice_feed(ctx.h, None, None, C.c_uint32(1), C.c_uint32(4)) == EINVAL
        ctx.tune(16, 1); ctx.upload(d["x"]); ctx.tune(16, 0)
        ctx.front()                                                          # between front and run the state belongs to that run
        recs, cnt = packed([[], []])
        assert ctx.lib.m17hip_voice_feed(ctx.h, recs.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.c_uint32(2), C.c_uint32(PITCH)) == ESTATE
        ctx.run()
    finally:
        ctx.tune(34, 0)
    ctx.upload(d["x"]); ctx.reset(); ctx.run()
    assert raw_voice(ctx, E2E_C, 10)[0] == ESTATE and raw_calls(ctx, 4)[0] == ESTATE
    ptrs = [C.c_void_p() for _ in range(3)]
    assert ctx.lib.m17hip_voice_device(ctx.h, C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]), C.byref(C.c_uint32(0))) == ESTATE
    recs, cnt = packed([[]])
    assert ctx.lib.m17hip_voice_feed(ctx.h, recs.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.c_uint32(PITCH)) == ESTATE
    off = ctx.frames()
    assert off.tobytes() == on.tobytes() == d["flat"].tobytes()
