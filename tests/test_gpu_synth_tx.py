"""GPU: m17hip_synth_tx_i16 — transmissions whose LSF and payload rows the caller supplies, synthesised on the device (mod_symbols_tx_kernel, one
wave per frame, then the unchanged shaper).  Held, int16 for int16, against the built-in generator on its own truth (m17hip_synth_i16 and the test
generator), against the CPU builder of tests/tx_build.py on content of its own, and through the demodulator against the oracle — with
FrameType::FULL_PACKET end to end, which no other input of the suite reaches."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import spliced as sp
import tx_build as tb

pytestmark = pytest.mark.gpu

MAXC, MAXT = 65, 96000
EINVAL, ESTATE = -1, -4
# (generator kind, payload frames): every kind at 0 (where it exists), 1, 6, 7 and 33 frames
COMBOS = ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1), (4, 1), (0, 6), (1, 6), (4, 6), (1, 7), (2, 7), (0, 7), (4, 7), (0, 33), (1, 33), (2, 33),
          (4, 33))


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(MAXC, MAXT)
    yield c
    c.close()


def raw_call(ctx, base, tx, lsf, rows, n_rows, channels, samples, chan0=0):
    """The C call itself (Context.synth_tx only ever builds descriptors that are in order); pointers may be None."""
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data_as(C.c_void_p))
    return ctx.lib.m17hip_synth_tx_i16(ctx.h, None if base is None else C.byref(base), p(tx), p(lsf), p(rows), C.c_uint32(n_rows),
                                       C.c_uint32(channels), C.c_uint32(samples), C.c_uint32(chan0))


def arrays_of(transmissions):
    """(tx, lsf, rows) as Context.synth_tx lays them out."""
    tx = np.zeros(len(transmissions), dtype=m17hip.TX_DTYPE)
    lsf = np.zeros((len(transmissions), 30), dtype=np.uint8)
    rows = []
    for i, (kind, l, frames) in enumerate(transmissions):
        tx[i] = (kind, len(frames), len(rows), 0)
        if l is not None:
            lsf[i] = np.frombuffer(bytes(l), dtype=np.uint8)
        rows += [bytes(r).ljust(32, b"\0") for r in frames]
    return tx, lsf, np.frombuffer(b"".join(rows), dtype=np.uint8).copy() if rows else np.zeros(32, dtype=np.uint8)


def in_place(ctx, base, transmissions, samples, chan0=0):
    ctx.synth_tx(base, transmissions, samples, chan0)
    return ctx.download()


def staged(ctx, base, transmissions, samples, chan0=0):
    """With tuning key 16 the call writes the staging slab: the run that follows makes it the current one."""
    ctx.tune(16, 1)
    try:
        ctx.synth_tx(base, transmissions, samples, chan0)
    finally:
        ctx.tune(16, 0)
    ctx.run()
    return ctx.download()


# ---- same truth, same bits ---------------------------------------------------------------------------------------------------------------------
#        channels, chan0, first combo, samples, key 16, what differs from the generator's defaults
CASES = {"one_clean_phase0": (1, 0, 10, 20000, False, dict(phase=0)),
         "three_far_noisy_inverted_staged": (3, 1000, 15, 72000, True,
                                             dict(noise_sigma=600.0, tail_sigma=600.0, dc_offset=350.0, gain=0.6, invert=1, lead_in=2688, lead_sigma=30000.0)),
         "wave_of_64_noisy": (64, 0, 0, 72000, False, dict(noise_sigma=600.0, tail_sigma=100.0, lead_in=2688)),
         "65_far_clean_gain_phase7_staged": (65, 1000, 5, 72000, True, dict(dc_offset=-200.0, gain=1.3, invert=1, phase=7, n_preamble=3))}


@pytest.mark.parametrize("name", list(CASES))
def test_generator_truth_gives_the_generators_slab(ctx, name):
    channels, chan0, first, T, key16, kw = CASES[name]
    seed = 6050 + len(name)
    combo = [COMBOS[(first + c) % len(COMBOS)] for c in range(channels)]
    exp = np.zeros((channels, T), dtype=np.int16)
    transmissions = []
    for c, (kind, nf) in enumerate(combo):
        x, truth = ol.generate(ol.gen_params(seed=tb.channel_seed(seed, chan0 + c), kind=kind, n_frames=nf, total=T, **kw), with_truth=True)
        exp[c] = x
        transmissions.append(tb.from_truth(kind, truth, nf))
        assert np.array_equal(ol.generate_batch(ol.gen_params(seed=seed, kind=kind, n_frames=nf, **kw), 1, T, threads=1, chan0=chan0 + c)[0], x), c
    base = ol.gen_params(seed=seed, kind=3, n_frames=12345, **kw)          # (kind and n_frames of the block are ignored)
    got = in_place(ctx, base, transmissions, T, chan0)
    assert got.shape == exp.shape and np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0][:8]
    ctx.run()
    if key16:
        assert np.array_equal(staged(ctx, base, transmissions, T, chan0), exp)
    for kind, nf in sorted(set(combo)):                                     # ... and m17hip_synth_i16's own slab
        ctx.synth(ol.gen_params(seed=seed, kind=kind, n_frames=nf, **kw), channels, T, chan0)
        own = ctx.download()
        for c in range(channels):
            if combo[c] == (kind, nf):
                assert np.array_equal(own[c], exp[c]), (kind, nf, c)


# ---- own content -----------------------------------------------------------------------------------------------------------------------------------
CALLS = ("", "N0CALL", "AB1CDE-9", "W1AW/P", "A.B-C/D12", "Z", "SP5WWP", "ABCDEFGHI")


def own_transmissions(seed, channels, frames_of):
    """Channel c: BERT (random bits, not PRBS9), a stream or a packet with callsigns, type field and rows of its own."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(channels):
        kind, n = c % 3, frames_of(c)
        if kind == tb.BERT:
            out.append((kind, None, [bytes(rng.integers(0, 256, 24, dtype=np.uint8)) + bytes([int(rng.integers(0, 32)) << 3]) for _ in range(n)]))
        elif kind == tb.STREAM:
            lsf = m17hip.make_lsf(CALLS[c % 8], CALLS[(c + 3) % 8], 0x0005 | (c % 16) << 7, bytes(rng.integers(0, 256, 14, dtype=np.uint8)))
            out.append((kind, lsf, [m17hip.stream_row(i, rng.integers(0, 256, 16, dtype=np.uint8), last=i == n - 1) for i in range(n)]))
        else:
            lsf = m17hip.make_lsf(CALLS[(c + 1) % 8], CALLS[(c + 5) % 8], (0x0002, 0x0004, 0x0006, 0x0000)[(c // 3) % 4])
            out.append((kind, lsf, [bytes(rng.integers(0, 256, 25, dtype=np.uint8)) + bytes([0x80 | 25 << 2 if i == n - 1 else i << 2]) for i in range(n)]))
    return out


def oracle_of(x):
    recs, counts, diags = ol.demod_batch(x, cap=2 * (x.shape[1] // 1920 + 2) + 4, threads=8)
    flat = np.concatenate([recs[c, :counts[c]] for c in range(x.shape[0])]) if counts.sum() else recs[0, :0]
    return flat, counts, diags


DIAG_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames", "evm", "deviation", "offset", "clock", "dcd_level")


def run_and_compare(ctx, x):
    exp, counts, diags = oracle_of(x)
    ctx.reset()
    ctx.run()
    got = ctx.frames()
    assert got.size == exp.size and got.tobytes() == exp.tobytes()
    d = ctx.diag(x.shape[0])
    for f in DIAG_FIELDS:
        assert np.array_equal(d[f], diags[f], equal_nan=True), f
    return got, d


@pytest.mark.parametrize("sigma", [0.0, 600.0])
def test_own_content_is_what_the_builder_makes_and_what_the_oracle_decodes(ctx, sigma):
    channels, T = 12, 40000
    transmissions = own_transmissions(77, channels, lambda c: 4 + c)
    # (seed 1: with it the oracle acquires all twelve transmissions behind the loud lead-in; searched once on the CPU)
    base = ol.gen_params(seed=1, lead_in=3072, lead_sigma=40000.0, noise_sigma=sigma, tail_sigma=max(sigma, 100.0))
    x = in_place(ctx, base, transmissions, T)
    assert np.array_equal(x, tb.batch(base, transmissions, T))
    got, _ = run_and_compare(ctx, x)
    if sigma == 0.0:                                                        # what was put in comes out
        for c, (kind, lsf, rows) in enumerate(transmissions):
            r = got[got["channel"] == c]
            n, want = {tb.BERT: (25, sp.FT_BERT), tb.STREAM: (18, sp.FT_STREAM), tb.PACKET: (26, None)}[kind]
            pay = r[r["frame_type"] != sp.FT_LSF] if kind != tb.STREAM else r[r["frame_type"] == sp.FT_STREAM]
            assert [bytes(q["payload"][:n]) for q in pay][:len(rows)] == [bytes(row[:n]) for row in rows], c
            if kind != tb.BERT:
                assert r[0]["frame_type"] == sp.FT_LSF and bytes(r[0]["payload"][:30]) == lsf, c


def test_full_packet_end_to_end(ctx):
    """FrameType::FULL_PACKET / State::FULL_PACKET (M17FrameDecoder.h:113-136, 379-386): an LSF whose type is not 0x0002 in front of packet frames."""
    channels, T = 16, 75000
    types = (0x0004, 0x0006, 0x0000, 0x0002)
    frames = (1, 2, 3, 5, 8, 12, 16, 20, 24, 27, 29, 30, 31, 32, 33, 33)
    rng = np.random.default_rng(4)
    transmissions = [(tb.PACKET, m17hip.make_lsf("", CALLS[1 + c % 7], types[c % 4]),
                      [bytes(rng.integers(0, 256, 25, dtype=np.uint8)) + bytes([0x80 | 25 << 2 if i == frames[c] - 1 else i << 2]) for i in range(frames[c])])
                     for c in range(channels)]
    # (seed 1: the oracle acquires all sixteen; searched once on the CPU.  Behind a transmission's EOT the noise may still yield LICH or BERT
    #  records: the assertions below are on the records of the transmission, the comparison with the oracle on all of them)
    base = ol.gen_params(seed=1, lead_in=3072, lead_sigma=40000.0, noise_sigma=200.0, tail_sigma=200.0)
    ctx.tune(7, 64)
    try:
        x = in_place(ctx, base, transmissions, T)
        got, diag = run_and_compare(ctx, x)
        packets = ctx.packets()
    finally:
        ctx.tune(7, 0)
    _, _, diags = oracle_of(x)
    assert np.array_equal(diag["demod_state"], diags["demod_state"])
    for c, (_, lsf, rows) in enumerate(transmissions):
        r = got[got["channel"] == c]
        want = sp.FT_BASIC_PACKET if types[c % 4] == 0x0002 else sp.FT_FULL_PACKET
        assert r["frame_type"].tolist()[:1 + len(rows)] == [sp.FT_LSF] + [want] * len(rows), (c, r["frame_type"].tolist())
        assert bytes(r[0]["payload"][:30]) == lsf and [bytes(q["payload"][:26]) for q in r[1:1 + len(rows)]] == rows, c
        exp = ol.PacketAssembler().feed(r["frame_type"], r["payload"])
        g = packets[packets["channel"] == c]
        assert len(exp) == g.size, (c, len(exp), g.size)
        for e, q in zip(exp, g):
            assert (int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"])) == (e["size"], e["checksum"], e["frames"], e["seq_errors"]), c
            assert np.array_equal(q["data"], e["data"]) and int(q["sample_pos"]) == int(r["sample_pos"][e["rec_index"]]), c
    assert packets.size >= channels // 2


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_burst_longer_than_the_slab_is_cut(ctx):
    transmissions = own_transmissions(78, 6, lambda c: 9 + c)
    base = ol.gen_params(seed=902, lead_in=100, noise_sigma=150.0)
    full = in_place(ctx, base, transmissions, 40000)
    for T in (5 * 1920 + 7, 1920, 333):                                    # mid-frame, inside the LSF frame, inside the preamble
        short = [(k, l, r[:T // 1920 + 1]) for k, l, r in transmissions]   # (n_frames beyond samples / 1920 + 1 are refused)
        assert np.array_equal(in_place(ctx, base, short, T), full[:, :T]), T


def test_nothing_behind_the_rows_is_read(ctx):
    transmissions = own_transmissions(79, 5, lambda c: 3 + c)
    tx, lsf, rows = arrays_of(transmissions)
    n_rows = rows.size // 32
    assert int(tx["first_row"][-1] + tx["n_frames"][-1]) == n_rows          # the last transmission ends with the buffer
    base = ol.gen_params(seed=903, noise_sigma=0.0)
    slabs = []
    for fill in (0x00, 0xFF, 0x5A):
        buf = np.full(rows.size + 4096, fill, dtype=np.uint8)               # the rows, then a guard region of ours
        buf[:rows.size] = rows
        assert raw_call(ctx, base, tx, lsf, buf, n_rows, 5, 20000) == 0
        ctx.C, ctx.T = 5, 20000
        slabs.append(ctx.download())
    assert np.array_equal(slabs[0], slabs[1]) and np.array_equal(slabs[0], slabs[2])
    assert np.array_equal(slabs[0], tb.batch(base, transmissions, 20000))
    # ... nor the padding of a row (bytes the frame does not carry), nor the bits of its last byte that are not sent
    dirty = []
    for kind, l, frames in transmissions:
        n, mask = {tb.BERT: (25, 0x07), tb.STREAM: (18, 0x00), tb.PACKET: (26, 0x03)}[kind]
        dirty.append((kind, l, [bytes(r[:n - 1]) + bytes([r[n - 1] | mask]) + b"\xa5" * (32 - n) for r in frames]))
    assert np.array_equal(in_place(ctx, base, dirty, 20000), slabs[0])


def test_refusals_leave_the_slab_alone(ctx):
    transmissions = own_transmissions(80, 4, lambda c: 2 + c)
    base = ol.gen_params(seed=904, noise_sigma=100.0)
    T = 20000
    before = in_place(ctx, base, transmissions, T)
    tx, lsf, rows = arrays_of(transmissions)
    n_rows = rows.size // 32

    def changed(field, c, value):
        t = tx.copy()
        t[field][c] = value
        return t

    bad = {"base NULL": (None, tx, lsf, rows, n_rows, 4, T), "tx NULL": (base, None, lsf, rows, n_rows, 4, T),
           "rows NULL": (base, tx, lsf, None, n_rows, 4, T), "lsf NULL with a stream": (base, tx, None, rows, n_rows, 4, T),
           "kind 3": (base, changed("kind", 2, 3), lsf, rows, n_rows, 4, T), "kind 2^31": (base, changed("kind", 0, 1 << 31), lsf, rows, n_rows, 4, T),
           "reserved": (base, changed("reserved", 1, 1), lsf, rows, n_rows, 4, T),
           "rows overrun by one": (base, tx, lsf, rows, n_rows - 1, 4, T),
           "first_row wraps": (base, changed("first_row", 3, 0xFFFFFFFF), lsf, rows, n_rows, 4, T),
           "too many frames": (base, changed("n_frames", 0, T // 1920 + 2), lsf, np.zeros(32 * 64, np.uint8), 64, 4, T),
           "no channels": (base, tx, lsf, rows, n_rows, 0, T), "no samples": (base, tx, lsf, rows, n_rows, 4, 0),
           "channels beyond the context": (base, np.resize(tx, MAXC + 1), np.resize(lsf, (MAXC + 1, 30)), rows, n_rows, MAXC + 1, T),
           "samples beyond the context": (base, tx, lsf, rows, n_rows, 4, MAXT + 1)}
    for what, args in bad.items():
        assert raw_call(ctx, *args) == EINVAL, what
        assert np.array_equal(ctx.download(), before), what
    # the last frame count that is allowed, and BERT alone without LSFs
    ok = changed("n_frames", 0, T // 1920 + 1)
    ok["first_row"][0] = 0
    assert raw_call(ctx, base, ok, lsf, np.zeros(32 * 64, np.uint8), 64, 4, T) == 0
    assert raw_call(ctx, base, np.array([(0, 2, 0, 0)], dtype=m17hip.TX_DTYPE), None, rows, n_rows, 1, T) == 0
    # between m17hip_demod_front and its run the slabs belong to that run
    ctx.C, ctx.T = 4, T
    before = in_place(ctx, base, transmissions, T)
    ctx.reset()
    ctx.run()
    ctx.tune(16, 1)
    try:
        ctx.synth_tx(base, transmissions, T)
    finally:
        ctx.tune(16, 0)                                                     # (no tuning between front and run either)
    ctx.front()
    try:
        assert raw_call(ctx, base, tx, lsf, rows, n_rows, 4, T) == ESTATE
        assert np.array_equal(ctx.download(), before)
    finally:
        ctx.run()
    assert np.array_equal(ctx.download(), before)                           # (the staged slab, now the current one: the same transmissions)


def test_the_staging_grows_and_is_reused(ctx):
    c2 = m17hip.Context(8, MAXT)                                            # (a context of its own: its staging starts empty)
    try:
        base = ol.gen_params(seed=905, noise_sigma=80.0, lead_in=500)
        for seed, nf, T in ((1, 2, 12000), (2, 40, 90000), (3, 1, 9000), (4, 40, 90000)):
            transmissions = own_transmissions(seed, 6, lambda c: nf if c != 2 else max(nf - 1, 1))
            c2.synth_tx(base, transmissions, T)
            assert np.array_equal(c2.download(), tb.batch(base, transmissions, T)), (nf, T)
    finally:
        c2.close()
