"""GPU tests of the host-side call orders around a context's FIRST stream change (findings 1 and 2): which bytes a fetch reads
when the stream that carries it changes while a run is still on the device.

A context that runs in place does a run's payload work (deferred decode, consumers) on the main stream.  From its first staged input on
(m17hip_upload_i16_async, m17hip_upload_i16_device_async, or tuning key 16 and an in-place producer) the fetch family —
m17hip_frames_count / _fetch / _compact_device, m17hip_bert_stats, m17hip_packets_fetch, the gather — works on the copy stream instead;
m17hip_set_stream moves everything that follows to a stream of the host's.  Every case here makes such a change with run 0 still in flight,
makes the call under test at once (no synchronisation in between), compares what it returns with the oracle byte for byte, then continues
the stream with run 1 and checks that run too.  Every case has a FRESH context: the change under test is the first one.

Run 0 is 4096 channels x 96 000 samples: 7.4-8.6 ms on the MI355X from m17hip_demod_run to the end of its work on the main stream (measured
once, six fresh contexts, events on that stream), against 0.1-3 ms on the host for the staging call that follows it (15 ms for the first
staging of a process).  Against the library without the ordering these cases fail with counts and records of a run still being written
(a fetch of run 0's 183 072 records returned 0-122 515 of them).  The "tiny" staging is one 1920-sample frame per channel (a
continued stream keeps its channel count, so a run 1 of fewer channels is refused): a copy that takes no time.  The full chunk is the next
24 000 samples of every channel."""
import ctypes as C
import itertools

import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

CN, T0, T1, TINY = 4096, 96000, 24000, 1920
CAP = 2 * ((T0 + T1) // 1920 + 2) + 4      # oracle record slots per channel
THREADS = 16

# the diagnostics of ONE run from a reset, compared as test_gpu_parity.py::test_full_chain_bit_exact compares them ...
DIAG_EXACT = ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
DIAG_FLOAT = ("evm", "deviation", "offset", "clock", "dcd_level")
# ... and those of a continued stream, as tests/test_gpu_streaming.py compares them
DIAG_STREAM = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "evm", "deviation", "offset", "clock")


def _params(seed, kind, n_frames, lead_in=3072, sigma=600.0):
    return ol.gen_params(seed=seed, kind=kind, n_frames=n_frames, lead_in=lead_in, noise_sigma=sigma, tail_sigma=sigma, lead_sigma=40000.0,
                         total=T0 + T1)


def _flat(recs, lo, hi):
    return np.concatenate([recs[c, lo[c]: hi[c]] for c in range(recs.shape[0])])


class Stream:
    """CN channels of T0 + T1 samples and the oracle's view of them: run 0 = the first T0 samples, run 1 = the next T1 ("full") or TINY
    ("tiny") samples of every channel.  The demodulator is causal: run 0's records are the first records of the whole stream, run 1's the rest."""

    def __init__(self, x, params=None, consumers=False):
        import torch
        self.x, self.params = x, params
        r0, n0, self.diag0 = ol.demod_batch(x[:, :T0], cap=CAP, threads=THREADS)
        self.rec0 = _flat(r0, np.zeros_like(n0), n0)
        self.rec1, self.diag1, rows1 = {}, {}, {}
        for name, t in (("full", T1), ("tiny", TINY)):
            r, n, d = ol.demod_batch(x[:, :T0 + t], cap=CAP, threads=THREADS)
            assert all(r[c, : n0[c]].tobytes() == r0[c, : n0[c]].tobytes() for c in range(CN)), name
            self.rec1[name], self.diag1[name] = _flat(r, n0, n), d
            rows1[name] = [r[c, : n[c]] for c in range(CN)]
        assert self.rec0.size > 10 * CN and self.rec1["full"].size > CN
        self.x0 = np.ascontiguousarray(x[:, :T0])
        self.x1 = {"full": np.ascontiguousarray(x[:, T0:]), "tiny": np.ascontiguousarray(x[:, T0:T0 + TINY])}
        self.pin1 = {k: torch.from_numpy(v).pin_memory() for k, v in self.x1.items()}
        self.dev = torch.from_numpy(x).cuda()           # [CN][T0 + T1]: run 0 = columns [0, T0), the chunk after it = columns [T0, ...)
        self.recbuf = torch.empty(CN * CAP * m17hip.FRAME_REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                         # (the producers' buffers are complete before they are handed over: include/m17hip.h)
        if consumers:
            rows0 = [r0[c, : n0[c]] for c in range(CN)]
            self.bert0 = _bert(rows0)
            self.bert1 = {k: _bert(v) for k, v in rows1.items()}
            self.pk0, self.pk1 = [], {"full": [], "tiny": []}
            for c in range(CN):
                for name in ("full", "tiny"):
                    a = ol.PacketAssembler()
                    p0 = _assemble(a, rows0[c])
                    p1 = _assemble(a, rows1[name][c][n0[c]:])
                    if name == "full":
                        self.pk0.append(p0)
                    self.pk1[name].append(p1)
            assert sum(map(len, self.pk0)) > CN // 8 and sum(map(len, self.pk1["full"])) > CN // 8


def _assemble(asm, recs):
    out = asm.feed(recs["frame_type"], recs["payload"]) if recs.size else []
    for e in out:
        e["pos"] = int(recs[e["rec_index"]]["sample_pos"])
    return out


def _bert(rows):
    out = np.zeros(len(rows), dtype=[("bits", "<u4"), ("errors", "<u4"), ("synced", "?"), ("frames", "<u4")])
    for c, r in enumerate(rows):
        b = r[r["frame_type"] == 5]
        bits, errs, sync = ol.bert_count(b["payload"][:, :25]) if b.size else (0, 0, False)
        out[c] = (bits, errs, sync, b.size)
    return out


@pytest.fixture(scope="module")
def voice():
    """Voice, BERT and packet channels as the generator mixes them (kind -1), one parameter block: m17hip_synth_i16 makes the same slab."""
    p = _params(seed=20261016, kind=-1, n_frames=55)
    return Stream(ol.generate_batch(p, CN, T0 + T1, threads=THREADS), params=p)


@pytest.fixture(scope="module")
def consumers():
    """BERT channels (clean and with bit errors) and packet channels (packets that close in run 0, and packets begun in run 0 that close in
    run 1), for the PRBS9 and packet consumers (tuning keys 6 and 7)."""
    q = CN // 4
    x = np.concatenate([ol.generate_batch(_params(seed=611, kind=0, n_frames=55), q, T0 + T1, threads=THREADS),
                        ol.generate_batch(_params(seed=612, kind=0, n_frames=55, sigma=2600.0), q, T0 + T1, threads=THREADS, chan0=q),
                        ol.generate_batch(_params(seed=613, kind=4, n_frames=20), q, T0 + T1, threads=THREADS, chan0=2 * q),
                        ol.generate_batch(_params(seed=614, kind=4, n_frames=12, lead_in=84000, sigma=400.0), q, T0 + T1, threads=THREADS,
                                          chan0=3 * q)])
    return Stream(x, consumers=True)


# ---- the steps of a case ---------------------------------------------------------------------------------------------------------
def _produce(ctx, s, producer):
    """Run 0's input, written in place."""
    if producer == "upload":
        ctx.upload(s.x0)
    elif producer == "upload_device":
        ctx.upload_device(s.dev.data_ptr(), CN, T0, pitch=T0 + T1)
    else:
        ctx.synth(s.params, CN, T0)
        assert np.array_equal(ctx.download(), s.x0)


STAGES = ("async_tiny", "async_full", "device_async", "tune16_upload")
CHUNK = {"async_tiny": "tiny", "async_full": "full", "device_async": "full", "tune16_upload": "tiny"}


def _stage(ctx, s, stage):
    """The context's first staged input: the chunk after run 0."""
    if stage == "async_tiny":
        ctx.upload_async(s.pin1["tiny"].data_ptr(), CN, TINY)
    elif stage == "async_full":
        ctx.upload_async(s.pin1["full"].data_ptr(), CN, T1)
    elif stage == "device_async":
        ctx.upload_device_async(s.dev.data_ptr() + 2 * T0, CN, T1, pitch=T0 + T1)
    else:
        ctx.tune(16, 1)
        ctx.upload(s.x1["tiny"])


def _frames_once(ctx):
    """m17hip_frames_fetch ONCE with room for every record (Context.frames repeats a fetch that was too small, and a repeat comes late)."""
    recs = np.zeros(CN * CAP, dtype=m17hip.FRAME_REC)
    got = C.c_uint64(0)
    ctx._chk(ctx.lib.m17hip_frames_fetch(ctx.h, m17hip._ptr(recs), C.c_uint64(recs.size), C.byref(got)))
    return recs[: got.value]


def _compact_device(ctx, s):
    n = ctx.frames_compact_device(s.recbuf.data_ptr(), CN * CAP)
    return s.recbuf[: n * m17hip.FRAME_REC.itemsize].cpu().numpy().view(m17hip.FRAME_REC)


def _check_diag(d, exp, fields):
    for f in fields:
        assert np.array_equal(d[f], exp[f], equal_nan=True), f


def _check_records(got, exp):
    assert got.size == exp.size, (got.size, exp.size)
    assert got.tobytes() == exp.tobytes()


def _check_bert(st, exp):
    assert np.array_equal(st["bits"], exp["bits"]) and np.array_equal(st["errors"], exp["errors"])
    assert np.array_equal(st["synced"] != 0, exp["synced"]) and np.array_equal(st["frames"], exp["frames"])


def _check_packets(got, exp):
    """As test_gpu_parity.py's consumer tests compare them: per channel, in order, every field and the payload."""
    assert got.size == sum(map(len, exp)), (got.size, sum(map(len, exp)))
    ch = got["channel"]
    for c, lst in enumerate(exp):
        g = got[ch == c]
        assert g.size == len(lst), c
        for e, q in zip(lst, g):
            assert (int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"])) == (e["size"], e["checksum"], e["frames"], e["seq_errors"]), c
            assert np.array_equal(q["data"], e["data"]) and bool(q["crc_ok"]) == (e["checksum"] == 0x0F47), c
            assert int(q["sample_pos"]) == e["pos"], c


def _call(ctx, s, call, after, chunk):
    """The call under test, checked against what the run it names (the selected run; m17_diag and the PRBS9 counts: the latest) holds."""
    latest_diag, latest_fields = (s.diag1[chunk], DIAG_STREAM) if after == "run_select1" else (s.diag0, DIAG_EXACT + DIAG_FLOAT)
    if call == "frames_count":
        assert ctx.frames_count() == s.rec0.size
    elif call == "frames":
        _check_records(_frames_once(ctx), s.rec0)
    elif call == "compact_device":
        _check_records(_compact_device(ctx, s), s.rec0)
    elif call == "diag":
        _check_diag(ctx.diag(CN), latest_diag, latest_fields)
    elif call == "bert_stats":
        _check_bert(ctx.bert_stats(CN), s.bert1[chunk] if after == "run_select1" else s.bert0)
    else:
        _check_packets(ctx.packets(capacity=4 * CN), s.pk0)


def _case(s, producer, stage, call, after, keys=()):
    ctx = m17hip.Context(CN, T0)
    try:
        for k in keys:
            ctx.tune(k, CN if k == 7 else 1)
        chunk = CHUNK[stage]
        t = TINY if chunk == "tiny" else T1
        _produce(ctx, s, producer)
        ctx.run()
        _stage(ctx, s, stage)                           # run 0 is still on the device: nothing in between synchronises
        if after == "front":
            ctx.front(channels=CN, samples=t)
        elif after == "run_select1":
            ctx.run(channels=CN, samples=t)
            ctx.frames_select(1)
        _call(ctx, s, call, after, chunk)
        # the stream goes on: run 1 on the staged chunk, then every fetch once more
        if after != "run_select1":
            ctx.run(channels=CN, samples=t)
        ctx.frames_select(1)
        _check_records(_frames_once(ctx), s.rec0)
        ctx.frames_select(0)
        assert ctx.frames_count() == s.rec1[chunk].size
        _check_records(_frames_once(ctx), s.rec1[chunk])
        _check_records(_compact_device(ctx, s), s.rec1[chunk])
        _check_diag(ctx.diag(CN), s.diag1[chunk], DIAG_STREAM)
        if 6 in keys:
            _check_bert(ctx.bert_stats(CN), s.bert1[chunk])
        if 7 in keys:
            _check_packets(ctx.packets(capacity=4 * CN), s.pk1[chunk])
        ctx.upload_wait()
    finally:
        ctx.close()


AFTERS = ("direct", "front", "run_select1")


def _matrix(calls, producers):
    """Every (call, what follows the staging) pair twice, with two different stagings; the producer and the staging rotate so that every
    (producer, staging) pair is met."""
    out = []
    for shift in (0, 2):
        for i, (call, after) in enumerate(itertools.product(calls, AFTERS)):
            producer, stage = producers[i % len(producers)], STAGES[(i + shift) % len(STAGES)]
            out.append(pytest.param(producer, stage, call, after, id=f"{producer}-{stage}-{call}-{after}"))
    return out


@pytest.mark.parametrize("producer,stage,call,after", _matrix(("frames_count", "frames", "compact_device", "diag"), ("upload", "upload_device", "synth")))
def test_fetch_right_after_the_first_staging(voice, producer, stage, call, after):
    """Run 0 in place, the first staging at once, then (directly, behind a front end of run 1, or behind run 1 with run 0 selected) a fetch:
    it names run 0 and must wait for it, on whichever stream it is queued."""
    _case(voice, producer, stage, call, after)


@pytest.mark.parametrize("producer,stage,call,after", _matrix(("bert_stats", "packets"), ("upload", "upload_device")))
def test_consumers_right_after_the_first_staging(consumers, producer, stage, call, after):
    """The same with the BERT and packet consumers on (tuning keys 6 and 7 before run 0): the PRBS9 counts (every run's consumer adds to
    them) and the packets of the selected run."""
    _case(consumers, producer, stage, call, after, keys=(6, 7))


@pytest.mark.parametrize("then", ["diag_frames", "run_next", "reset_run"])
@pytest.mark.parametrize("target", ["torch_stream", "null_stream"])
@pytest.mark.parametrize("staged", [False, True], ids=["in_place", "staged"])
def test_set_stream_with_a_run_in_flight(voice, staged, target, then):
    """m17hip_set_stream at once after run 0 was queued on the library's stream: what follows on the new stream (a fetch, the next run with
    the state carried, a reset and a run from scratch) is ordered behind run 0.  `staged`: the context has staged input before (tuning key 16
    and an in-place upload: its payload stream is the copy stream), or not (the payload stream is the main stream and moves with it)."""
    import torch
    s = voice
    side = torch.cuda.Stream() if target == "torch_stream" else None
    ctx = m17hip.Context(CN, T0)
    try:
        if staged:
            ctx.tune(16, 1)
        ctx.upload(s.x0)
        ctx.run()
        ctx.set_stream(side.cuda_stream if side is not None else 0)
        assert ctx.stream == (side.cuda_stream if side is not None else 0)
        if then == "diag_frames":
            _check_diag(ctx.diag(CN), s.diag0, DIAG_EXACT + DIAG_FLOAT)
            _check_records(_frames_once(ctx), s.rec0)
        elif then == "run_next":
            ctx.upload(s.x1["full"])
            ctx.run()
            _check_records(_frames_once(ctx), s.rec1["full"])
            _check_diag(ctx.diag(CN), s.diag1["full"], DIAG_STREAM)
            ctx.frames_select(1)
            _check_records(_frames_once(ctx), s.rec0)
        else:
            ctx.reset()
            ctx.upload(s.x0)
            ctx.run()
            _check_records(_frames_once(ctx), s.rec0)
            _check_diag(ctx.diag(CN), s.diag0, DIAG_EXACT + DIAG_FLOAT)
    finally:
        ctx.close()
        torch.cuda.synchronize()
