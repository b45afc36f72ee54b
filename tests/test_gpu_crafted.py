"""GPU: the chain below the matched filter on CRAFTED matched-filter output.  m17hip_set_fir_taps (include/m17hip.h, a test hook) puts the identity into
the context's tap tables (tap 0 = 1, the rest 0); on a float32 stream y[n] == x[n] then, and a test writes sample by sample what the correlator, the sync
search, the level estimator and the sequential kernel's slicer see.  Below the filter the reference is full of exact float comparisons — find_peak's
strict > on fabs scanned in buffer order, the high / low split of outer_symbol_levels around hi + lo/2. with its count == 0 fallbacks — which the
sequential kernel runs lane-parallel with ballots where the oracle is scalar; an RRC-filtered waveform never produces a tie or a degenerate level set.

One Context(64, 48000), identity taps, float32 rows (tests/crafted_lib.py).  Every batch in one run and in runs of 1920 samples, with key 15 = 0 (every
frame decoded where it completes) and key 17 = 0 as further cells: records as bytes, every callback of the diagnostic log and the final m17_diag
against the oracle whose Fir150 holds the same taps (tests/cxx/crafted_oracle.cpp), no tolerance.  tests/test_crafted.py asserts on the oracle alone
that each batch contains what it is about."""
import numpy as np
import pytest

import crafted_lib as cl
import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BATCHES = ("natural", "held", "levels", "exact", "small", "long_ties")
CELLS = {"one_run": (cl.CR_T, {}), "runs_of_1920": (1920, {}), "decode_in_place": (cl.CR_T, {15: 0}), "key17_off": (cl.CR_T, {17: 0}),
         "runs_of_1920_decode_in_place": (1920, {15: 0})}
DEFAULTS = {15: 1, 17: 1, 6: 0, 7: 0}
FT_BERT = 5


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(64, cl.CR_T)      # (long_ties has 32 channels, rounding 20)
    c.set_fir_taps(cl.IDENTITY)
    yield c
    c.close()


def test_identity_taps_pass_the_row_through(ctx):
    """y[n] == x[n], as words: zeros, negative zeros and subnormals included (every other product is 0 x finite = +-0, and adding it changes nothing but
    the sign of a zero sum, which the oracle's Fir150 shares)."""
    x = cl.natural()[:33, :3841].copy()
    x[0, 100:110] = np.float32(1e-40)
    x[1, 200:210] = np.float32(-0.0)
    ctx.reset()
    ctx.upload(x)
    y = ctx.fir()
    e = cl.fir(x, cl.IDENTITY)
    assert np.array_equal(y.view(np.uint32), e.view(np.uint32))
    nz = x != 0
    assert np.array_equal(y[nz].view(np.uint32), x[nz].view(np.uint32))


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("name", BATCHES)
def test_crafted_batch(ctx, name, cell):
    L, keys = CELLS[cell]
    x, r = getattr(cl, name)(), cl.oracle_of(name)
    for k, v in keys.items():
        ctx.tune(k, v)
    try:
        cl.check_stream(ctx, x, r, L, f"{name}, {cell}")
    finally:
        for k in keys:
            ctx.tune(k, DEFAULTS[k])


@pytest.mark.parametrize("cell", ["one_run", "runs_of_1920", "decode_in_place"])
def test_rounding_rows_under_the_rrc_taps(ctx, cell):
    """int16 transmissions on which ClockRecovery's std::round sees x.5 exactly (tests/test_crafted.py), under the RRC taps restored on the same
    context; the identity goes back in behind the cell."""
    L, keys = CELLS[cell]
    ctx.set_fir_taps(None)
    for k, v in keys.items():
        ctx.tune(k, v)
    try:
        cl.check_stream(ctx, cl.rounding(), cl.rounding_oracle(), L, f"rounding, {cell}")
    finally:
        for k in keys:
            ctx.tune(k, DEFAULTS[k])
        ctx.reset()
        ctx.set_fir_taps(cl.IDENTITY)


@pytest.mark.parametrize("name", ("natural", "held", "levels"))
def test_consumers_on_crafted_rows(ctx, name):
    """The BERT statistics (key 6) and the packet reassembly (key 7) over one run of the batch, against their CPU twins fed the oracle's records."""
    x, r = getattr(cl, name)(), cl.oracle_of(name)
    ctx.tune(6, 1)
    ctx.tune(7, 4096)
    try:
        ctx.reset()
        ctx.upload(x)
        ctx.run()
        assert ctx.frames().tobytes() == r.frames().tobytes()
        st = ctx.bert_stats(64)
        got = ctx.packets(capacity=4096)
        exp, n_bert = [], 0
        for c in range(64):
            recs = r.recs[c, : r.counts[c]]
            pay = recs[recs["frame_type"] == FT_BERT]["payload"][:, :25]
            bits, errs, sync = ol.bert_count(pay) if pay.size else (0, 0, False)
            assert (int(st["bits"][c]), int(st["errors"][c]), bool(st["synced"][c]), int(st["frames"][c])) == (bits, errs, sync, pay.shape[0]), (name, c)
            n_bert += pay.shape[0]
            for e in ol.PacketAssembler().feed(recs["frame_type"], recs["payload"]):
                exp.append((c, e["size"], e["checksum"], e["frames"], e["seq_errors"], int(recs["sample_pos"][e["rec_index"]]), e["data"]))
        # (held: a tie moves the sample index off the symbol, the payload no longer decodes as what was sent and the channels end in BERT frames — no packets)
        assert n_bert >= 64 and len(exp) >= (0 if name == "held" else 8), (name, n_bert, len(exp))
        assert got.size == len(exp), (name, got.size, len(exp))
        for q, e in zip(got, exp):
            assert (int(q["channel"]), int(q["size"]), int(q["checksum"]), int(q["frames"]), int(q["seq_errors"]), int(q["sample_pos"])) == e[:6], (name, e[:6])
            assert np.array_equal(q["data"], e[6]), (name, e[0])
    finally:
        ctx.tune(6, 0)
        ctx.tune(7, 0)
