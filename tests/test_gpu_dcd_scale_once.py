"""K3 (sliding-DFT carrier detect) with its samples scaled in the packed f32 form (both polarities, head and tail included): the
table of sums against the oracle bit for bit at the shapes where a partial wave, shadow lanes, a second workgroup, the ragged head
and tail, the wrap of a 128-sample delay and a tick boundary can go wrong, in both forms of the kernel; continuation across ragged
launches; and one two-segment full chain, whose second K3 launch takes its delayed samples from the first segment's."""
import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

CMAX, TMAX = 65, 1000
LENGTHS = (31, 32, 119, 120, 121, 191, 192, 193, 992, 1000)   # 992 = 31 whole blocks: the latency form on more than one tick


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(CMAX, 96000)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table_case():
    """Full-range input (both int16 extremes among it: the inverted polarity wraps -32768) and the oracle's sums for every table
    cell of the longest length; shorter lengths are prefixes of the same rows.  Computed once, never modified."""
    rng = np.random.default_rng(20261017)
    x = rng.integers(-32768, 32768, size=(CMAX, TMAX), dtype=np.int64).astype(np.int16)
    x[:, 5::97] = -32768
    x[:, 11::89] = 32767
    ticks = TMAX // 192
    exp = np.zeros((2, CMAX, ticks, 2, 6), dtype=np.float32)
    for inv in (0, 1):
        for c in range(CMAX):
            xs = ol.scale(x[c], invert=inv)
            for k in range(ticks):
                for j in range(6):
                    # sum j restarts with the ticks = j (mod 5); before its first restart, and sum 5 always, it runs from the stream start
                    a0 = 0 if j == 5 else max(k - ((k - j) % 5), 0)
                    exp[inv, c, k, :, j] = ol.dcd_sums(xs, 192 * a0, 192 * (k - a0 + 1))
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("C", [1, 33, 65])
def test_dcd_table_equals_oracle_sums(ctx, table_case, C, invert):
    x, exp = table_case
    for form in (0, 1):   # key 10: the one-wave form / the four-wave pipeline wherever the length allows it
        ctx.tune(10, form)
        try:
            for T in LENGTHS:
                ctx.upload(x[:C, :T])
                sums = ctx.dcd(flags=m17hip.FLAG_INVERT if invert else 0)
                assert sums.shape == (C, T // 192, 2, 6)
                assert np.array_equal(sums.view(np.uint32), exp[invert, :C, : T // 192].view(np.uint32)), (form, T)
        finally:
            ctx.tune(10, -1)


@pytest.fixture(scope="module")
def stream_case():
    C, T = 33, 9600
    p = ol.gen_params(seed=1017, kind=-1, n_frames=3, lead_in=1200, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=T)
    x = ol.generate_batch(p, C, T, threads=8)
    recs, counts, diags = ol.demod_batch(x, cap=16, threads=8)
    flat = np.concatenate([recs[c, : counts[c]] for c in range(C)]) if counts.sum() else recs[0, :0]
    x.setflags(write=False)
    return x, flat, diags


def _run_chunks(ctx, x, chunks):
    ctx.reset()
    parts, pos = [], 0
    for n in chunks:
        ctx.upload(x[:, pos: pos + n])
        ctx.run()
        parts.append(ctx.frames().copy())
        pos += n
    assert pos == x.shape[1]
    got = np.concatenate(parts)
    return got[np.lexsort((got["seq"], got["channel"]))], ctx.diag().copy()


@pytest.mark.parametrize("form", [0, 1])
def test_ragged_launches_continue_the_delay_line(ctx, stream_case, form):
    """100 + 1000 + 37 samples == one launch of 1137: the launches start inside a block (pos0 = 100, 1100), are seeded from the
    carried x prefix, and feed head and tail through the same delay.  The carrier-detect level at the first update point (2304
    samples) sums every sample since the stream start, so the runs that follow (15 samples up to a block boundary, then 8448 = 264
    whole blocks, which the forced latency form takes) carry what the ragged launches left to where it shows."""
    x, exp, diags = stream_case
    ctx.tune(10, form)
    try:
        got_a, d_a = _run_chunks(ctx, x, (100, 1000, 37, 15, 8448))
        got_b, d_b = _run_chunks(ctx, x, (1137, 15, 8448))
    finally:
        ctx.tune(10, -1)
    assert got_a.tobytes() == got_b.tobytes() == exp.tobytes()
    assert d_a.tobytes() == d_b.tobytes()
    for f in ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d_a[f], diags[f]), f
    assert np.array_equal(d_a["dcd_level"], diags["dcd_level"], equal_nan=True)
    assert (diags["n_diag"] > 0).all()   # the level was updated: K3's sums were read


def test_full_chain_two_segments_default_knobs(ctx):
    """64 channels x 96 000 samples = two 48 000-sample segments: the second K3 launch takes its delayed samples from the first
    segment's.  Records and m17_diag against the oracle."""
    C, T = 64, 96000
    p = ol.gen_params(seed=1018, kind=-1, n_frames=T // 1920 - 4, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=T)
    x = ol.generate_batch(p, C, T, threads=8)
    recs, counts, diags = ol.demod_batch(x, cap=2 * (T // 1920 + 2) + 4, threads=8)
    exp = np.concatenate([recs[c, : counts[c]] for c in range(C)])
    ctx.upload(x)
    ctx.reset()
    ctx.run()
    got = ctx.frames()
    assert got.size == exp.size and got.size > C
    assert got.tobytes() == exp.tobytes()
    d = ctx.diag()
    for f in ("dcd", "locked", "sample_index", "sync_index", "clock_index", "viterbi_cost", "n_diag", "demod_state", "n_frames"):
        assert np.array_equal(d[f], diags[f]), f
    for f in ("evm", "deviation", "offset", "clock", "dcd_level"):
        assert np.array_equal(d[f], diags[f], equal_nan=True), f
