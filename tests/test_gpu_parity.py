"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against the CPU
oracle on identical seeded inputs.  Integer / decision outputs must be bit-exact; the float operator outputs
are compared bit-exact as well (the north star allows 1e-5 relative — we assert the stronger property and
report the looser one only if it ever fails)."""
import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _signals(C, T, seed=77, sigma=500.0, kind=-1, lead_in=3072):
    p = ol.gen_params(seed=seed, kind=kind, n_frames=max(1, T // 1920 - 4), lead_in=lead_in, noise_sigma=sigma, tail_sigma=sigma,
                      lead_sigma=40000.0, total=T)
    return ol.generate_batch(p, C, T, threads=8)


def _oracle_records(x, invert=0):
    recs, counts, diags = ol.demod_batch(x, invert=invert, cap=2 * (x.shape[1] // 1920 + 2) + 4, threads=8)
    flat = np.concatenate([recs[c, : counts[c]] for c in range(x.shape[0])]) if counts.sum() else recs[0, :0]
    return flat, counts, diags


@pytest.fixture(scope="module", params=[(1, -1, 0, 1), (0, -1, 0, 0), (1, 1, 1, 1)], ids=["default", "decode_and_evm_in_k5", "k3_latency_form_redo_in_front"])
def ctx(request):
    """Every test runs three times: with the payload frames of running transmissions decoded after the run, one lane per frame (the default),
    with every frame decoded by the sequential kernel's wave where it completes (m17hip_tune key 15 = 0), and with the carrier-detect
    kernel K3 in its four-wave latency form (key 10 = 1; by default only the runs m17hip_demod_front queues use it)."""
    c = m17hip.Context(256, 96000)
    c.tune(15, request.param[0])
    c.tune(10, request.param[1])
    c.tune(20, request.param[2])   # the replay's redo beside K5 (default) / in front of it with the history stored
    c.tune(17, request.param[3])   # the running EVM folded outside K5 (default) / inside it
    yield c
    c.close()


def test_scale_exhaustive(ctx):
    """All 65536 int16 values through K1's scaling: a FIR whose window holds one sample isolates tap*x."""
    s = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    # place each value alone, 200 samples apart -> y at the value's position = x * taps[0] (+0 terms)
    x = np.zeros((16, 4096 * 200), dtype=np.int16)
    x = x[:, :96000]
    vals = s.reshape(16, 4096)[:, :480]
    x[:, ::200] = vals
    ctx.upload(x)
    y = ctx.fir()
    exp = np.stack([ol.fir_i16(x[c]) for c in range(16)])
    assert np.array_equal(y, exp)
    yi = ctx.fir(flags=m17hip.FLAG_INVERT)
    expi = np.stack([ol.fir_i16(x[c], invert=1) for c in range(16)])
    assert np.array_equal(yi, expi)
    # and every one of the 65536 values: K3 scales x[n] and x[n-120] itself -> compare the DFT sums on a ramp
    ramp = np.tile(s, 2)[:96000][None, :].repeat(2, axis=0)
    ramp[1] = ramp[1][::-1]
    ctx.upload(ramp)
    for flags in (0, m17hip.FLAG_INVERT):   # ... and through K1: all values, both polarities
        assert np.array_equal(ctx.fir(flags=flags), np.stack([ol.fir_i16(ramp[c], invert=flags) for c in range(2)]))
    sums = ctx.dcd()
    for c in range(2):
        xs = ol.scale(ramp[c])
        for k in (0, 11, 100, 499):
            a = ol.dcd_sums(xs, 192 * k, 192)
            assert (float(sums[c, k, 0, k % 5]), float(sums[c, k, 1, k % 5])) == (float(a[0]), float(a[1]))


def test_fir_bit_exact_and_ragged(ctx):
    x = _signals(24, 40000, seed=5)
    for T in (40000, 3841, 3839, 150, 149, 1):
        ctx.upload(x[:, :T])
        y = ctx.fir()
        exp = np.stack([ol.fir_i16(x[c, :T]) for c in range(x.shape[0])])
        assert np.array_equal(y, exp), T
    rel = 0.0  # documented tolerance of the north star (1e-5 relative) is implied by bit equality


def test_correlator_bit_exact(ctx):
    x = _signals(12, 30000, seed=6, sigma=800.0)
    ctx.upload(x)
    y = ctx.fir()
    limit, corr = ctx.correlator()
    for c in range(x.shape[0]):
        l, k = ol.correlator(y[c])
        assert np.array_equal(limit[c], l), c
        assert np.array_equal(corr[:, c, :], k), c


def test_iir_denormal_decay(ctx):
    """The limit IIR must not flush denormals: a burst followed by exact zeros decays through the subnormal range."""
    x = np.zeros((2, 90000), dtype=np.int16)
    x[:, :300] = 20000
    ctx.upload(x)
    y = ctx.fir()
    limit, _ = ctx.correlator()
    l, _ = ol.correlator(y[0])
    assert np.array_equal(limit[0], l)
    assert (np.abs(l[l != 0]) < 1.2e-38).any(), "test input never reached the subnormal range"


def test_dcd_table_bit_exact(ctx):
    x = _signals(6, 24000, seed=9, sigma=300.0)
    ctx.upload(x)
    sums = ctx.dcd()
    rng = np.random.default_rng(0)
    for c in range(x.shape[0]):
        xs = ol.scale(x[c])
        # first update point of the reference: samples [0, 2304)
        a = ol.dcd_sums(xs, 0, 2304)
        assert (float(sums[c, 11, 0, 5]), float(sums[c, 11, 1, 5])) == (float(a[0]), float(a[1]))
        for _ in range(12):
            k = int(rng.integers(12, sums.shape[1]))
            span = int(rng.choice([2, 5, 1, 3]))
            a0 = k - span + 1
            e = ol.dcd_sums(xs, 192 * a0, 192 * span)
            assert (float(sums[c, k, 0, a0 % 5]), float(sums[c, k, 1, a0 % 5])) == (float(e[0]), float(e[1])), (c, k, span)


def test_slicer_and_evm_bit_exact(ctx, golden):
    """llr<float,4> incl. every float within +-64 ulp of each of the 43 table edges, and the running EVM."""
    import ctypes as C
    edges = np.zeros(43, dtype=np.float32); l0 = np.zeros(43, np.int8); l1 = np.zeros(43, np.int8)
    ol.oracle().m17o_llr_table(ol._p(edges), ol._p(l0), ol._p(l1))
    near = []
    for e in edges:
        v = np.float32(e)
        lo = v
        for _ in range(64):
            lo = np.nextafter(lo, np.float32(-10))
        cur = lo
        for _ in range(129):
            near.append(cur)
            cur = np.nextafter(cur, np.float32(10))
    rng = np.random.default_rng(2)
    sym = np.concatenate([np.array(near, np.float32), golden["llr_in"], rng.normal(0, 2.5, 50000).astype(np.float32),
                          np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, -3.0, 1e-45], np.float32)])
    sym = np.concatenate([sym, np.zeros((-sym.size) % 8, np.float32)]).reshape(8, -1)
    llr, evm = ctx.slice_llr(sym)
    for r in range(8):
        assert np.array_equal(llr[r].reshape(-1), ol.llr(sym[r])), r
        assert np.array_equal(evm[r], ol.evm_trace(sym[r], 1), equal_nan=True), r


def test_viterbi_bit_exact(ctx, golden):
    rng = np.random.default_rng(4)
    for kind, (IN, OUT) in m17hip.VITERBI_SHAPES.items():
        soft = rng.integers(-7, 8, (200, IN)).astype(np.int8)
        # half of them: valid codewords with a few errors, punctured positions erased
        for i in range(0, 200, 2):
            bits = rng.integers(0, 2, OUT).astype(np.uint8)
            enc = ol.conv_encode(bits).astype(np.int16) * 2 - 1
            s = enc * rng.integers(1, 8, IN)
            s = np.where(rng.random(IN) < 0.04, -s, s)
            s[rng.random(IN) < 0.1] = 0
            soft[i] = s.astype(np.int8)
        bits, cost = ctx.viterbi(soft, kind)
        for i in range(200):
            c, out = ol.viterbi(soft[i], OUT)
            assert c == cost[i] and np.array_equal(out, bits[i]), (kind, i)
    # the reference's own LSF known-answer vector (tests/ViterbiTest.cpp:173-195)
    exp = np.array(golden["kat"]["lsf_expected240"], dtype=np.uint8)
    enc = np.array(golden["kat"]["lsf_encoded488"], dtype=np.int16)
    enc[11] = 1
    bits, cost = ctx.viterbi((enc * 14 - 7).astype(np.int8)[None, :], 0)
    assert cost[0] == 0 and np.array_equal(bits[0], exp)


def test_decode_frames_golden_sequences(ctx, golden):
    """The frame decoder (K4') against the sequences recorded from the reference's own M17FrameDecoder."""
    state = {}
    for e in golden["kat"]["frame_decoder_sequences"]:
        st = state.get(e["seed"], (0, 0, np.zeros(30, np.uint8), 0, 0))
        recs, nrec, s, li, lsf, d401, cost = ctx.decode_frames(np.array(e["llr"], np.int8), [e["st"]], [st[0]], [st[1]], st[2][None, :],
                                                               [st[3]], [st[4]])
        state[e["seed"]] = (int(s[0]), int(li[0]), lsf[0], int(d401[0]), int(cost[0]))
        assert (int(s[0]), int(li[0]), lsf[0].tolist(), int(d401[0]), int(cost[0])) == (e["state"], e["lich"], e["lsf"], e["d401"], e["cost"])
        got = [(int(r["frame_type"]), int(r["cost"]), int(r["len"]), bytes(r["payload"]).hex()) for r in recs[0, : nrec[0]]]
        assert got == [tuple(v) for v in e["recs"]]


def test_decode_frames_random_walk_batch(ctx):
    rng = np.random.default_rng(23)
    frames = []
    for kind in (0, 1, 2):
        fb, st = ol.make_frames(kind, 300 + kind, 6)
        frames += [(int(t), b) for t, b in zip(st, fb)]
    n = 192
    so = [(0, 0, np.zeros(30, np.uint8), 0, 0) for _ in range(n)]
    for step in range(12):
        llr = np.zeros((n, 368), np.int8); sts = np.zeros(n, np.uint8)
        for i in range(n):
            t, b = frames[rng.integers(len(frames))]
            if rng.random() < 0.15:
                t = int(rng.integers(0, 4))
            fr = (b.astype(np.int16) * 2 - 1) * rng.integers(1, 8, 368)
            llr[i] = np.where(rng.random(368) < rng.choice([0.0, 0.03, 0.3]), -fr, fr).astype(np.int8)
            sts[i] = t
        recs, nrec, s, li, lsf, d401, cost = ctx.decode_frames(llr, sts, [v[0] for v in so], [v[1] for v in so], np.stack([v[2] for v in so]),
                                                               [v[3] for v in so], [v[4] for v in so])
        for i in range(n):
            ro = ol.decode_frame(int(sts[i]), llr[i], *so[i])
            so[i] = ro[1:]
            assert (ro[1], ro[2], ro[3].tolist(), ro[4], ro[5]) == (int(s[i]), int(li[i]), lsf[i].tolist(), int(d401[i]), int(cost[i])), (step, i)
            a = ro[0].copy(); b = recs[i, : nrec[i]].copy()
            a["channel"] = 0; b["channel"] = 0; a["seq"] = 0; b["seq"] = 0
            assert a.tobytes() == b.tobytes(), (step, i)


@pytest.mark.parametrize("seed,sigma,kind,invert", [(1, 0.0, 0, 0), (2, 400.0, -1, 0), (3, 1500.0, -1, 0), (4, 2500.0, 1, 1), (5, 800.0, 2, 0)])
def test_full_chain_bit_exact(ctx, seed, sigma, kind, invert):
    C, T = 64, 48000
    x = _signals(C, T, seed=seed, sigma=sigma, kind=kind)
    ctx.upload(x)
    ctx.reset()
    ctx.run(flags=invert)
    got = ctx.frames()
    exp, counts, diags = _oracle_records(x, invert=invert)
    assert got.size == exp.size
    assert got.tobytes() == exp.tobytes()
    d = ctx.diag()
    for f in ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    for f in ("evm", "deviation", "offset", "clock", "dcd_level"):
        assert np.array_equal(d[f], diags[f], equal_nan=True), f
    if sigma <= 800:
        assert got.size > C  # the test does decode frames


def test_full_chain_clean_bert_anchor(ctx):
    """a clean BERT burst decodes to the PRBS9 payloads with cost 0 — on the GPU."""
    s, truth = ol.generate(ol.gen_params(seed=1, kind=0, n_frames=6, phase=0), with_truth=True)
    ctx.upload(np.stack([s, s]))
    ctx.reset()
    ctx.run()
    recs = ctx.frames()
    assert recs.size == 12
    for i, r in enumerate(recs[:6]):
        assert r["frame_type"] == 5 and r["cost"] == 0 and bytes(r["payload"][:25]) == bytes(truth["payloads"][i][:25])
    assert bytes(recs[0]["payload"][:25]).hex() == "08c272ac37a6e450ad3f6496fc9a9980c651a5fd163acb3c78"


def test_full_chain_streaming_chunks_equal_one_shot(ctx):
    """Runs continue from the carried state: 5 chunks of 9600 == one run of 48000 (and == the oracle)."""
    C, T = 64, 48000
    x = _signals(C, T, seed=12, sigma=600.0)
    exp, counts, _ = _oracle_records(x)
    ctx.reset()
    parts = []
    for k in range(5):
        ctx.upload(x[:, 9600 * k: 9600 * (k + 1)])
        ctx.run()
        parts.append(ctx.frames().copy())
    got = np.concatenate(parts)
    order = np.lexsort((got["seq"], got["channel"]))
    assert got[order].tobytes() == exp.tobytes()


def test_full_chain_ragged_chunks(ctx):
    """Chunk lengths that are not multiples of 8 / 192 / 1920 (unaligned DCD blocks, FIR tiles, bulk chunks)."""
    C, T = 32, 40000
    x = _signals(C, T, seed=31, sigma=700.0)
    exp, counts, diags = _oracle_records(x)
    ctx.reset()
    parts, pos = [], 0
    for n in (1, 7, 149, 1919, 3841, 9601, 12345, 5000, T):
        n = min(n, T - pos)
        if n <= 0:
            break
        ctx.upload(x[:, pos: pos + n])
        ctx.run()
        parts.append(ctx.frames().copy())
        pos += n
    assert pos == T
    got = np.concatenate(parts)
    order = np.lexsort((got["seq"], got["channel"]))
    assert got[order].tobytes() == exp.tobytes()
    d = ctx.diag()
    for f in ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    assert np.array_equal(d["dcd_level"], diags["dcd_level"], equal_nan=True)


def test_full_chain_lost_sync_drops_limit_speculation(ctx):
    """A burst followed by noise: the carrier detect stays on, sync is lost, the demodulator forces dcd.unlock() — the one
    event K2's gate replay cannot foresee.  The run must drop the speculative filter history there and stay bit-exact."""
    C, T = 32, 48000
    p = ol.gen_params(seed=41, kind=-1, n_frames=6, lead_in=3072, noise_sigma=500.0, tail_sigma=3000.0, lead_sigma=40000.0, total=T)
    x = ol.generate_batch(p, C, T, threads=8)
    exp, counts, diags = _oracle_records(x)
    ctx.upload(x)
    ctx.reset()
    ctx.run()
    got = ctx.frames()
    dropped = ctx.replay_drops()
    assert got.tobytes() == exp.tobytes() and got.size > C
    d = ctx.diag()
    for f in ("dcd", "locked", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    assert np.array_equal(d["dcd_level"], diags["dcd_level"], equal_nan=True)
    assert dropped >= C // 2, dropped   # the scenario does exercise the fallback: most channels left the replay at least once
    # ... and the next runs (fresh speculation from the saved state) continue bit-exact: same input as two chunks
    ctx.reset()
    parts = []
    for a, b in ((0, 30000), (30000, T)):
        ctx.upload(x[:, a:b])
        ctx.run()
        parts.append(ctx.frames().copy())
    got2 = np.concatenate(parts)
    order = np.lexsort((got2["seq"], got2["channel"]))
    assert got2[order].tobytes() == exp.tobytes()


@pytest.mark.parametrize("seg", [0, 7001, 19200])
def test_full_chain_run_in_segments(ctx, seg):
    """Tuning knob 3: a run is processed as K2+K5 segments (fresh limit-filter speculation per segment); any segment length,
    aligned or not, gives the same records and diagnostics."""
    C, T = 48, 60000
    p = ol.gen_params(seed=52, kind=-1, n_frames=9, lead_in=3072, noise_sigma=700.0, tail_sigma=2500.0, lead_sigma=40000.0, total=T)
    x = ol.generate_batch(p, C, T, threads=8)
    exp, counts, diags = _oracle_records(x)
    ctx.tune(3, seg)
    try:
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got = ctx.frames()
        d = ctx.diag()
    finally:
        ctx.tune(3, 48000)
    assert got.tobytes() == exp.tobytes() and got.size > C
    for f in ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    for f in ("evm", "deviation", "offset", "clock", "dcd_level"):
        assert np.array_equal(d[f], diags[f], equal_nan=True), f


def test_full_chain_two_bursts_across_segments(ctx):
    """Burst, noise (sync lost: forced unlock, the limit speculation is dropped), second burst — processed in 9600-sample
    segments, so the second burst is acquired and decoded on filter history that K2 REDID from K5's state after the drop."""
    C, T = 32, 72000
    a = ol.generate_batch(ol.gen_params(seed=61, kind=-1, n_frames=6, lead_in=3072, noise_sigma=500.0, tail_sigma=2500.0, lead_sigma=40000.0,
                                        total=36000), C, 36000, threads=8)
    b = ol.generate_batch(ol.gen_params(seed=62, kind=-1, n_frames=8, lead_in=2000, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=2500.0,
                                        total=36000), C, 36000, threads=8)
    x = np.concatenate([a, b], axis=1)
    exp, counts, diags = _oracle_records(x)
    second = exp[exp["sample_pos"] >= 36000] if "sample_pos" in exp.dtype.names else exp
    assert second.size > C   # the second burst does decode in the reference
    ctx.tune(3, 9600)
    try:
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got = ctx.frames()
        d = ctx.diag()
    finally:
        ctx.tune(3, 48000)
    assert got.tobytes() == exp.tobytes()
    for f in ("dcd", "locked", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    assert np.array_equal(d["dcd_level"], diags["dcd_level"], equal_nan=True)


@pytest.mark.parametrize("seed", [101, 202, 303])
def test_full_chain_random_scenarios(ctx, seed):
    """Randomised streams: every channel is two or three bursts of a random kind (BERT / voice / packet), length, noise level,
    lead-in loudness, DC offset, gain and symbol phase, separated by noise of random strength — acquisitions, lost syncs, carrier
    drops and re-acquisitions at uncorrelated positions.  Run in 19 200-sample segments; records and diagnostics bit-exact."""
    rng = np.random.default_rng(seed)
    C, T = 48, 96000
    x = np.zeros((C, T), dtype=np.int16)
    for c in range(C):
        pos = 0
        while pos < T - 8000:
            n = int(rng.integers(8000, 40000))
            n = min(n, T - pos)
            p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.integers(0, 3)), n_frames=int(rng.integers(2, 14)),
                              lead_in=int(rng.integers(0, 4000)), lead_sigma=float(rng.choice([0.0, 300.0, 3000.0, 40000.0])),
                              noise_sigma=float(rng.choice([0.0, 200.0, 800.0, 2000.0])), tail_sigma=float(rng.choice([0.0, 300.0, 3000.0])),
                              dc_offset=float(rng.choice([0.0, 0.0, 500.0, -1500.0])), gain=float(rng.choice([1.0, 0.5, 1.5])),
                              phase=int(rng.integers(-1, 10)), total=n)
            x[c, pos:pos + n] = ol.generate(p)[:n]
            pos += n
    exp, counts, diags = _oracle_records(x)
    assert exp.size > 4 * C
    ctx.tune(3, 19200)
    try:
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got = ctx.frames()
        d = ctx.diag()
    finally:
        ctx.tune(3, 48000)
    if got.tobytes() != exp.tobytes():
        n = min(got.size, exp.size)
        bad = sorted(set(int(exp[i]["channel"]) for i in range(n) if got[i].tobytes() != exp[i].tobytes()))
        raise AssertionError(f"records differ: sizes {got.size}/{exp.size}, channels {bad[:16]}")
    for f in ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    for f in ("evm", "deviation", "offset", "clock", "dcd_level"):
        assert np.array_equal(d[f], diags[f], equal_nan=True), f
    assert np.array_equal(d["pad"], diags["pad"])   # live clock / sync counters at the end of the run


@pytest.mark.parametrize("kw", [
    dict(seed=11, kind=-1, n_frames=20, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0),
    dict(seed=12, kind=0, n_frames=9, lead_in=0, noise_sigma=0.0, tail_sigma=0.0, phase=7),                       # zero noise: +-1 dither
    dict(seed=13, kind=1, n_frames=14, lead_in=2000, noise_sigma=1500.0, tail_sigma=300.0, dc_offset=-1500.0, gain=0.6, invert=1),
    dict(seed=14, kind=2, n_frames=11, lead_in=100, noise_sigma=200.0, tail_sigma=4000.0, dc_offset=2500.0, gain=1.4, n_preamble=3),
    dict(seed=15, kind=3, n_frames=0, lead_in=500, noise_sigma=900.0, tail_sigma=100.0, lead_sigma=12000.0),
    dict(seed=16, kind=4, n_frames=17, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0),   # packets closed by an FCS
])
def test_device_synthesis_bit_exact(ctx, kw):
    """m17hip_synth_i16 (m17-mod framing, RRC shaping in double, impairments) against the test generator: every
    int16 of the slab, several channel offsets; and the synthesized slab demodulates to the same records."""
    C, T = 40, 48000
    p = ol.gen_params(total=T, **kw)
    for chan0 in (0, 4093):
        exp = ol.generate_batch(p, C, T, threads=8, chan0=chan0)
        ctx.synth(p, C, T, chan0=chan0)
        got = ctx.download()
        assert np.array_equal(got, exp), (kw, chan0, int((got != exp).sum()))
    ctx.reset()
    ctx.run(flags=kw.get("invert", 0))
    recs = ctx.frames()
    e, counts, _ = _oracle_records(exp, invert=kw.get("invert", 0))
    assert recs.tobytes() == e.tobytes()
    if kw["kind"] != 3 and kw["noise_sigma"] <= 600.0:
        assert recs.size >= C // 2


def test_streaming_ingest_double_buffered(ctx):
    """m17hip_upload_i16_async stages the next run's input in a second slab while the current run computes; the
    carried tail moves with the swap.  Five runs fed that way == one run of the whole stream == the oracle."""
    import torch
    C, T, n = 64, 9600, 5
    x = _signals(C, n * T, seed=77, sigma=600.0)
    exp, counts, _ = _oracle_records(x)
    pinned = [torch.from_numpy(np.ascontiguousarray(x[:, k * T:(k + 1) * T])).pin_memory() for k in range(n)]
    ctx.reset()
    ctx.upload_async(pinned[0].data_ptr(), C, T)
    parts = []
    for k in range(n):
        ctx.run()                                   # consumes the staged slab (waits for its copy)
        if k + 1 < n:
            ctx.upload_async(pinned[k + 1].data_ptr(), C, T)   # overlaps with the run just queued
        parts.append(ctx.frames().copy())
    got = np.concatenate(parts)
    order = np.lexsort((got["seq"], got["channel"]))
    assert got[order].tobytes() == exp.tobytes() and got.size > C


def test_lsf_presentation_consumer(ctx):
    """LinkSetupFrame::decode_callsign + type + CRC on the device for a batch of LSFs: the LSF records of decoded
    voice / packet streams, plus random and corrupted frames, against the oracle."""
    x = np.stack([ol.generate(ol.gen_params(seed=900 + c, kind=1 + (c & 1), n_frames=5, lead_in=3072, lead_sigma=40000.0, noise_sigma=300.0,
                                            tail_sigma=300.0, total=24000))[:24000] for c in range(16)])
    ctx.upload(x); ctx.reset(); ctx.run()
    recs = ctx.frames()
    lsf = recs[recs["frame_type"] == 0]["payload"][:, :30]
    assert lsf.shape[0] >= 12
    rng = np.random.default_rng(3)
    rnd = rng.integers(0, 256, (500, 30), dtype=np.uint8)
    rnd[:50, :6] = 0xFF                     # broadcast destination
    bad = lsf.copy(); bad[:, 20] ^= 0x40    # CRC failures
    batch = np.concatenate([lsf, rnd, bad])
    info = ctx.lsf_info(batch)
    for i, f in enumerate(batch):
        assert bytes(info["dst"][i]).ljust(10, b"\0") == ol.decode_callsign(f[0:6]), i
        assert bytes(info["src"][i]).ljust(10, b"\0") == ol.decode_callsign(f[6:12]), i
        assert int(info["type"][i]) == (int(f[12]) << 8 | int(f[13]))
        assert bool(info["crc_ok"][i]) == (ol.crc16(f.tobytes()) == 0)
    n = lsf.shape[0]
    assert info["crc_ok"][:n].all() and not info["crc_ok"][-n:].any()
    assert bytes(info["src"][0]) == b"N0CALL" and bytes(info["dst"][0]) == b"BROADCAST"


def test_bert_statistics_consumer(ctx):
    """decode_bert + PRBS9::validate on the device (m17hip_bert_stats) against the oracle's PRBS9 receiver fed with the
    oracle's BERT frame payloads — noisy BERT bursts (bit errors, PRBS resynchronisations), the stream fed as two runs."""
    C, T = 48, 60000
    x = np.stack([ol.generate(ol.gen_params(seed=700 + c, kind=0, n_frames=24, lead_in=3072, lead_sigma=40000.0,
                                            noise_sigma=[300.0, 1500.0, 2600.0, 3400.0][c % 4], tail_sigma=500.0, total=T))[:T] for c in range(C)])
    recs, counts, _ = ol.demod_batch(x, cap=2 * (T // 1920 + 2) + 4, threads=8)
    ctx.tune(6, 1)
    try:
        ctx.reset()
        for a, b in ((0, 25000), (25000, T)):
            ctx.upload(x[:, a:b])
            ctx.run()
        st = ctx.bert_stats(C)
    finally:
        ctx.tune(6, 0)
    total_err = 0
    for c in range(C):
        r = recs[c, :counts[c]]
        pay = r[r["frame_type"] == 5]["payload"][:, :25]
        bits, errs, sync = ol.bert_count(pay) if pay.size else (0, 0, False)
        assert (int(st["bits"][c]), int(st["errors"][c]), bool(st["synced"][c]), int(st["frames"][c])) == (bits, errs, sync, pay.shape[0]), c
        total_err += errs
    assert total_err > 0 and int(st["frames"].sum()) > 10 * C   # the scenario has both decoded frames and bit errors
    with pytest.raises(m17hip.M17HipError):
        ctx.bert_stats(C)   # not enabled any more


def _check_packets(got, exp_by_channel, pos_by_channel=None):
    for c, exp in enumerate(exp_by_channel):
        g = got[got["channel"] == c]
        assert len(exp) == g.size, (c, len(exp), g.size)
        for e, q in zip(exp, g):
            assert (int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"])) == (e["size"], e["checksum"], e["frames"], e["seq_errors"]), c
            assert np.array_equal(q["data"], e["data"]) and bool(q["crc_ok"]) == (e["checksum"] == 0x0F47), c
            if pos_by_channel is not None:
                assert int(q["sample_pos"]) == int(pos_by_channel[c][e["rec_index"]]), c


def test_packet_reassembly_consumer(ctx):
    """decode_packet (apps/m17-demod.cpp:207-253) on the device (m17hip_packets_fetch) against the oracle's
    restatement fed with the oracle's frame records: one packet transmission per channel (with and without a frame check
    sequence, 1..33 frames, clean to very noisy so that frames are lost and checksums break), the stream fed as two runs so
    that half-assembled packets cross the run boundary."""
    C, T = 48, 90000
    import itertools
    cases = list(itertools.product([4, 4, 2], [300.0, 900.0, 1800.0, 2600.0], [1, 5, 33, 12]))   # kind x noise x frames = 48 channels
    x = np.stack([ol.generate(ol.gen_params(seed=9000 + c, kind=kind, n_frames=nf, lead_in=3072, lead_sigma=40000.0, noise_sigma=sigma,
                                            tail_sigma=400.0, total=T))[:T] for c, (kind, sigma, nf) in enumerate(cases)])
    recs, counts, _ = ol.demod_batch(x, cap=2 * (T // 1920 + 2) + 4, threads=8)
    ctx.tune(7, 1024)
    try:
        ctx.reset()
        got = []
        for a, b in ((0, 20000), (20000, T)):
            ctx.upload(x[:, a:b])
            ctx.run()
            got.append(ctx.packets())
        got = np.concatenate(got)
    finally:
        ctx.tune(7, 0)
    exp = [ol.PacketAssembler().feed(recs[c, :counts[c]]["frame_type"], recs[c, :counts[c]]["payload"]) for c in range(C)]
    _check_packets(got, exp, [recs[c]["sample_pos"] for c in range(C)])
    assert int(got["crc_ok"].sum()) >= C // 3 and int((got["crc_ok"] == 0).sum()) >= 4, (int(got["crc_ok"].sum()), got.size)
    assert got[got["crc_ok"] == 1]["size"].max() > 800      # a full-length (33-frame) packet made it through intact
    assert (got["sample_pos"] > 20000).sum() > C // 4         # ... closed in the second run, begun in the first
    with pytest.raises(m17hip.M17HipError):
        ctx.packets()   # not enabled any more


def test_packet_reassembly_rules_on_crafted_records(ctx):
    """The packet consumer over caller-supplied records (m17hip_packets_feed): random record sequences per channel — LSFs,
    numbered frames mostly but not always in sequence, closing frames with every byte count, other frame types in between —
    fed in three slices with the assembly state carried over, against the oracle's decode_packet restatement."""
    rng = np.random.default_rng(2024)
    C, N = 80, 90
    recs = np.zeros((C, N), dtype=m17hip.FRAME_REC)
    for c in range(C):
        counter, since_lsf = 0, 0
        for k in range(N):
            r = recs[c, k]
            r["channel"], r["seq"], r["sample_pos"] = c, k, 1920 * k + c
            u = rng.random()
            r["payload"][:26] = rng.integers(0, 256, 26, dtype=np.uint8)
            if u < 0.08 or since_lsf > 30:
                r["frame_type"], counter, since_lsf = 0, 0, 0
            elif u < 0.20:
                r["frame_type"] = int(rng.choice([1, 2, 5]))
            elif u < 0.32:                                                    # closing frame, any count (values above 25 are clamped)
                r["frame_type"], r["payload"][25] = int(rng.choice([3, 4])), 0x80 | (int(rng.integers(0, 32)) << 2) | int(rng.integers(0, 4))
                since_lsf += 1
            else:
                num = counter if rng.random() < 0.85 else int(rng.integers(0, 32))
                r["frame_type"], r["payload"][25] = int(rng.choice([3, 4])), (num << 2) | int(rng.integers(0, 4))
                counter += int(num == counter)
                since_lsf += 1
    ctx.tune(7, 4096)
    try:
        ctx.reset()
        got = []
        for a, b in ((0, 31), (31, 32), (32, N)):
            counts = np.full(C, b - a, dtype=np.uint32)
            counts[C - 1] = 0 if a == 31 else b - a                          # an empty row as well
            ctx.packets_feed(recs[:, a:b], counts)
            got.append(ctx.packets())
        got = np.concatenate(got)
    finally:
        ctx.tune(7, 0)
    exp = []
    for c in range(C):
        use = np.concatenate([recs[c, :31], recs[c, 31:32] if c != C - 1 else recs[c, :0], recs[c, 32:]])
        exp.append(ol.PacketAssembler().feed(use["frame_type"], use["payload"]))
    assert max(e["size"] for ex in exp for e in ex) <= 832
    _check_packets(got, exp)
    assert got.size > 5 * C and 0 < int((got["seq_errors"] > 0).sum()) < got.size


def test_packets_feed_after_the_payload_stream_has_moved():
    """m17hip_packets_feed works on the reassembly state the runs' own consumer leaves, so it goes behind every run's payload work wherever
    that was queued.  Here it was queued on the main stream (an in-place run) and the payload stream has moved to the copy stream since (the first
    staged input): one packet transmission per channel, every packet still open at the end of the run, closed by hand-made records through the
    feed.  The packets are those of the oracle's decode_packet restatement fed the run's records and then the closing ones."""
    import torch
    C, T = 16, 19200
    x = np.stack([ol.generate(ol.gen_params(seed=9100 + c, kind=(4, 4, 2)[c % 3], n_frames=(12, 20, 33, 16)[c % 4], lead_in=3072, lead_sigma=40000.0,
                                            noise_sigma=(300.0, 900.0)[c % 2], tail_sigma=400.0, total=2 * T))[:T] for c in range(C)])
    recs, counts, _ = ol.demod_batch(x, cap=2 * (T // 1920 + 2) + 4, threads=8)
    rng = np.random.default_rng(77)
    closing = np.zeros((C, 2), dtype=m17hip.FRAME_REC)   # odd channels: a numbered frame (in sequence or not) in front of the closing frame
    n_closing = np.array([1 + (c & 1) for c in range(C)], dtype=np.uint32)
    for c in range(C):
        for k in range(n_closing[c]):
            r = closing[c, k]
            r["channel"], r["seq"], r["sample_pos"], r["frame_type"] = c, int(counts[c]) + k, T + 1920 * k, 3 + (c >> 1 & 1)
            r["payload"][:26] = rng.integers(0, 256, 26, dtype=np.uint8)
            last = k + 1 == n_closing[c]
            in_seq = int(np.isin(recs[c, :counts[c]]["frame_type"], (3, 4)).sum())   # the number the run's frames lead up to (none was lost here)
            num = in_seq if c % 4 == 1 and not last else int(rng.integers(0, 32))
            r["payload"][25] = (0x80 if last else 0) | (num << 2) | int(rng.integers(0, 4))
    exp = []
    for c in range(C):
        asm = ol.PacketAssembler()
        assert asm.feed(recs[c, :counts[c]]["frame_type"], recs[c, :counts[c]]["payload"]) == []   # nothing closes within the run
        exp.append(asm.feed(closing[c, :n_closing[c]]["frame_type"], closing[c, :n_closing[c]]["payload"]))
    assert all(len(e) == 1 for e in exp) and sum(e[0]["frames"] > 4 for e in exp) >= C // 2   # ... and the run's frames are in the packets
    pinned = torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
    c2 = m17hip.Context(C, T)   # (a context that has never staged input: its payload stream is still the main stream)
    try:
        c2.tune(7, 64)
        c2.upload(x)
        c2.run()
        c2.upload_async(pinned.data_ptr(), C, T)   # the payload stream is the copy stream from here on
        c2.upload_wait()
        c2.packets_feed(closing, n_closing)
        got = c2.packets()
    finally:
        c2.close()
    _check_packets(got, exp)


def test_full_size_properties():
    """BASELINE config 3 at full size (4096 channels x 480 000 samples, synthesized on the device), checked through properties
    that need no oracle run: BERT channels -> the PRBS9 receiver locks and counts (almost) no errors over ~240 frames; voice
    channels -> one LSF, then stream frames whose frame numbers count up by one and end with the EOT flag; the first 32 channels
    bit-exact against the oracle."""
    C, T = 4096, 480000
    nf = T // 1920 - 6
    p = ol.gen_params(seed=20260101, kind=-1, n_frames=nf, lead_in=3072, noise_sigma=600.0, tail_sigma=600.0, lead_sigma=40000.0, total=T)
    c = m17hip.Context(C, T)
    try:
        c.tune(6, 1)
        c.synth(p, C, T)
        c.reset()
        c.run()
        recs = c.frames()
        st = c.bert_stats(C)
        x32 = c.download()[:32]
    finally:
        c.close()
    exp, counts, _ = _oracle_records(x32)
    assert recs[recs["channel"] < 32].tobytes() == exp.tobytes()
    bert = st[0::2]
    locked = bert["bits"] > 0.9 * 197 * nf
    assert locked.mean() > 0.9, locked.mean()   # (a few per cent of the channels acquire late or resynchronise the PRBS: reference behaviour)
    assert (bert["errors"][locked] / bert["bits"][locked]).mean() < 2e-3
    ok = 0
    for ch in range(1, 512, 2):                     # voice channels (a sample of them)
        r = recs[recs["channel"] == ch]
        s_ = r[r["frame_type"] == 2]
        if s_.size < nf - 2:
            continue
        fn = (s_["payload"][:, 0].astype(np.int32) << 8) | s_["payload"][:, 1]
        good = s_["cost"] < 30
        d = np.diff(fn[good] & 0x7FFF)
        assert (d[d > 0] >= 1).all() and (fn[-1] & 0x8000 or not good[-1])
        assert (r["frame_type"] == 0).sum() >= 1
        ok += 1
    assert ok > 190, ok   # (the others acquired late: fewer stream frames)


def test_edge_cases(ctx):
    # silence with +-1 dither, pure loud noise, DC, a stream cut in the middle of a frame, an all-zero window (NaN poisoning, Q1)
    T = 20000
    rng = np.random.default_rng(8)
    x = np.zeros((6, T), dtype=np.int16)
    x[0] = rng.choice([-1, 1], T)
    x[1] = np.clip(rng.normal(0, 20000, T), -32768, 32767).astype(np.int16)
    x[2] = 12000
    sig = ol.generate(ol.gen_params(seed=3, kind=0, n_frames=12, lead_in=3072, noise_sigma=300, lead_sigma=40000.0))
    x[3, :] = sig[:T]
    x[4, 5000:] = sig[: T - 5000]                     # exact zeros for 5000 samples first: DCD level becomes NaN forever
    x[5] = -32768
    ctx.upload(x)
    ctx.reset()
    ctx.run()
    got = ctx.frames()
    exp, counts, diags = _oracle_records(x)
    assert got.tobytes() == exp.tobytes()
    d = ctx.diag()
    assert np.array_equal(d["dcd_level"], diags["dcd_level"], equal_nan=True) and np.isnan(d["dcd_level"][4])


def test_cxx_drop_in_demodulator_app():
    """examples/m17-demod-gpu.cpp drives mobilinkd::M17Demodulator<float> (the mirror header) exactly as apps/m17-demod.cpp
    drives the reference: its frame callbacks must be the oracle's, in order."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    s = ol.generate(ol.gen_params(seed=5, kind=1, n_frames=12, lead_in=3072, noise_sigma=300.0, tail=4000, tail_sigma=300.0, lead_sigma=40000.0))
    out = subprocess.run([exe], input=s.tobytes(), capture_output=True, check=True).stdout.decode().split("\n")
    got = [l for l in out if l.strip()]
    recs, _ = ol.demod(s)
    exp = [f"{int(r['frame_type'])} {int(r['cost'])} {bytes(r['payload'][:r['len']]).hex()}" for r in recs]
    assert got == exp and len(exp) > 3


@pytest.mark.parametrize("seg", [4800, 9600, 48000])
def test_gate_aware_front_end_on_bursty_channels(seg):
    """m17hip_tune key 26 = 1 (NOTES 5.8): K1 of segment k >= 2 skips the tiles the carrier cannot be on for, forecast from K5's TRUE gate state
    at the end of segment k - 2 and K3's table.  Channels made of short transmissions of every kind between long stretches of loud, quiet
    and no noise (the gate closes by forced unlocks and reopens on the next preamble, at any place relative to the segments and to K1's
    tiles), 40 channels x 240 000 samples: records and diagnostics equal the oracle's, and equal the run with the gate-aware path off."""
    Cn, T = 40, 240000
    rng = np.random.default_rng(4242 + seg)
    x = np.zeros((Cn, T), dtype=np.int16)
    for c in range(Cn):
        pos = 0
        while pos < T - 9000:
            n = min(int(rng.integers(9000, 70000)), T - pos)
            p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.choice([0, 1, 2, 4])), n_frames=int(rng.integers(1, 9)),
                              lead_in=int(rng.integers(0, 6000)), lead_sigma=float(rng.choice([100.0, 20000.0, 40000.0])), noise_sigma=float(rng.choice([100.0, 600.0, 1500.0])),
                              tail_sigma=float(rng.choice([100.0, 5000.0, 20000.0])), phase=int(rng.integers(-1, 10)), total=n)
            x[c, pos:pos + n] = ol.generate(p)[:n]; pos += n
        x[c, pos:] = rng.integers(-300, 300, T - pos)
    recs, counts, diags = ol.demod_batch(x, cap=2 * (T // 1920 + 2) + 4, threads=8)
    exp = np.concatenate([recs[c, :counts[c]] for c in range(Cn)])
    ctx = m17hip.Context(Cn, T)
    ctx.tune(3, seg)
    outs = []
    for mode in (1, 0):
        ctx.tune(26, mode)
        ctx.upload(x); ctx.reset(); ctx.run()
        got = ctx.frames()
        assert got.tobytes() == exp.tobytes(), (seg, mode)
        d = ctx.diag(Cn)
        for f in ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "evm", "deviation", "offset", "clock", "dcd_level"):
            assert np.array_equal(d[f], diags[f], equal_nan=True), (seg, mode, f)
        outs.append(got.tobytes())
    assert outs[0] == outs[1]
    ctx.close()
