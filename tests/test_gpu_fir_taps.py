"""GPU tests of m17hip_set_fir_taps (ABI 614, include/m17hip.h: a test hook that rewrites the context's two matched-filter tap tables).  The RRC taps are
symmetric, h[i] == h[148 - i], so a tap index mirrored anywhere — in fs_build_tap_table or a K1 form that reads its table, in the sequential kernel's own
filter at a gate reopening, in K2's patch window, in the order of a carried history — computes the same words on every other test of the suite.  With
taps that are not symmetric it is a value error.

Everything is bit-exact against the oracle's Fir150 holding the same taps (tests/crafted_lib.py, tests/cxx/crafted_oracle.cpp): matched-filter outputs
as uint32 words, records as bytes, every callback of the diagnostic log and the final m17_diag.  The whole-chain premises (frames decode in both bursts;
most channels reopen the gate behind a carrier-off update point) are asserted on the oracle alone in tests/test_crafted.py."""
import ctypes as C

import numpy as np
import pytest

import crafted_lib as cl
import f32_lib as fl
import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
INV = m17hip.FLAG_INVERT
CS, TS = (1, 33), (1, 149, 150, 1041, 3841)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = m17hip.Context(max(CS), max(TS))
    yield c
    c.close()


# ---- operator level ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows():
    """int16 rows (never -32768: negation is then exact) with their floats, and float32 rows of small integers, |x| <= 15: with the ramp every product is
    an integer below 2^12 and every partial sum one below 2^19 — exact in float32 in any order, so a wrong index reads off the value."""
    rng = np.random.default_rng(614)
    xi = rng.integers(-32767, 32768, size=(max(CS), max(TS)), dtype=np.int16)
    xf = rng.integers(-15, 16, size=(max(CS), max(TS))).astype(np.float32)
    return {"int16": (xi, cl.scale(xi)), "float32": (xf, xf)}


TAP_SETS = {"delta0": cl.delta(0), "delta1": cl.delta(1), "delta74": cl.delta(74), "delta147": cl.delta(147), "delta148": cl.delta(148), "ramp": cl.ramp(),
            "random": cl.random_taps(6140)}


def _polarities(Cn):
    """(table or None, flag): plain, FLAG_INVERT, a mixed table, and the mixed table under FLAG_INVERT."""
    mixed = ((np.arange(Cn) * 5 // 3) & 1).astype(np.uint8) if Cn > 1 else np.ones(1, np.uint8)
    return [(None, 0), (None, INV), (mixed, 0), (mixed, INV)]


def _fir_cells(ctx, x, xf, taps, what):
    """Every shape and polarity form of m17hip_fir_rrc150 under the taps in force against Fir150 with `taps`."""
    for Cn in CS:
        exp = {p: cl.fir(xf[:Cn], taps, invert=p) for p in (0, 1)}   # y[t] depends on x[0 .. t] alone: a shorter slab's expectation is a prefix
        for T in TS:
            ctx.reset()
            ctx.upload(x[:Cn, :T])
            for tab, flag in _polarities(Cn):
                ctx.set_channel_polarity(tab)
                y = ctx.fir(flags=flag)
                for c in range(Cn):
                    p = (0 if tab is None else int(tab[c])) ^ (1 if flag else 0)
                    e = exp[p][c, :T]
                    bad = np.flatnonzero(_u32(y[c]) != _u32(e))
                    assert bad.size == 0, (what, Cn, T, "table" if tab is not None else "uniform", flag, c, int(bad[0]), float(y[c, bad[0]]), float(e[bad[0]]))
            ctx.set_channel_polarity(None)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", list(TAP_SETS))
def test_matched_filter_with_chosen_taps(ctx, rows, name, dtype):
    """A delta at tap k delays the row by k samples (k = 0, 1, 74, 147, 148: both ends of the table, its middle, and the neighbours of the ends); the ramp
    and a random set weigh every tap differently.  int16 and float32 rows, uniform plain, uniform inverted and a mixed polarity table, one channel and 33,
    slabs of 1, 149, 150, 1041 and 3841 samples."""
    x, xf = rows[dtype]
    taps = TAP_SETS[name]
    ctx.set_fir_taps(taps)
    try:
        if name.startswith("delta") and dtype == "float32":   # (what the oracle must say, said without it)
            k = int(name[5:])
            e = cl.fir(xf[:1], taps)[0]
            assert np.array_equal(e[k:], xf[0, : xf.shape[1] - k]) and not e[:k].any()
        _fir_cells(ctx, x, xf, taps, (name, dtype))
    finally:
        ctx.set_fir_taps(None)


def test_ramp_sums_are_exact(rows):
    """The ramp on small integers: the float32 result is the integer convolution, so the oracle itself is checked against int64 arithmetic here."""
    xf = rows["float32"][1][:3]
    e = cl.fir(xf, cl.ramp())
    t = np.arange(1, 150, dtype=np.int64)
    for c in range(3):
        full = np.convolve(xf[c].astype(np.int64), t)[: xf.shape[1]]
        assert np.array_equal(e[c].astype(np.int64), full) and np.array_equal(e[c], full.astype(np.float32))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_restored_taps_give_what_a_fresh_context_gives(ctx, rows, dtype):
    """NULL restores the RRC taps: the same words as before any call (a fresh context), which are the oracle's m17o_fir_*."""
    x, xf = rows[dtype]
    Cn, T = max(CS), max(TS)
    fresh = m17hip.Context(Cn, T)
    try:
        fresh.upload(x)
        before = fresh.fir()
    finally:
        fresh.close()
    ctx.set_fir_taps(cl.random_taps(6141))
    ctx.reset()
    ctx.upload(x)
    other = ctx.fir()
    ctx.set_fir_taps(None)
    after = ctx.fir()
    assert np.array_equal(_u32(after), _u32(before)) and not np.array_equal(_u32(other), _u32(before))
    exp = cl.fir(xf, ol.taps()[:149])
    assert np.array_equal(_u32(after), _u32(exp))
    assert np.array_equal(_u32(exp[0]), _u32(ol.fir_f32(xf[0])))
    _fir_cells(ctx, x, xf, ol.taps()[:149], ("restored", dtype))


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_fir_correlator_with_chosen_taps(ctx, rows, dtype):
    """m17hip_fir_correlator (K1 and K2 pipelined in time, K2's pieces reading what K1 wrote) under one asymmetric set: y against Fir150 with the set,
    the limit filter and the four correlations against the oracle's Correlator on that y."""
    x, xf = rows[dtype]
    taps = cl.random_taps(6142)
    ctx.set_fir_taps(taps)
    try:
        for Cn, T in ((1, 1041), (33, 3841)):
            ctx.reset()
            ctx.upload(x[:Cn, :T])
            y, limit, corr = ctx.fir_correlator()
            e = cl.fir(xf[:Cn, :T], taps)
            assert np.array_equal(_u32(y), _u32(e)), (Cn, T)
            for c in range(Cn):
                el, ec = ol.correlator(e[c])
                assert np.array_equal(_u32(limit[c]), _u32(el)) and np.array_equal(_u32(corr[:, c]), _u32(ec)), (Cn, T, c)
    finally:
        ctx.set_fir_taps(None)


def test_refusals(ctx, rows):
    """M17HIP_EINVAL for a NULL context or a tap that is not finite, M17HIP_ESTATE between m17hip_demod_front and its run; nothing changes then."""
    lib = m17hip.load_library()
    t = cl.ramp()
    assert lib.m17hip_set_fir_taps(C.c_void_p(), t.ctypes.data_as(C.c_void_p)) == EINVAL
    assert lib.m17hip_set_fir_taps(C.c_void_p(), None) == EINVAL
    x, xf = rows["float32"]
    ctx.set_fir_taps(t)
    try:
        for k, v in ((0, np.nan), (74, np.inf), (148, -np.inf)):
            bad = t.copy()
            bad[k] = v
            with pytest.raises(m17hip.M17HipError):
                ctx.set_fir_taps(bad)
        with pytest.raises(TypeError):
            ctx.set_fir_taps(np.zeros(150, np.float32))
        ctx.reset()
        ctx.upload(x[:1, :150])
        assert np.array_equal(_u32(ctx.fir()), _u32(cl.fir(xf[:1, :150], t)))      # the ramp is still in force
        # between front and run: a run is staged beside the one that exists, its front end queued
        import torch
        T = 960
        pin = torch.from_numpy(np.ascontiguousarray(x[:2, T:2 * T])).pin_memory()
        ctx.reset()
        ctx.upload(x[:2, :T])
        ctx.run()
        ctx.upload_async(pin.data_ptr(), 2, T, dtype=np.float32)
        ctx.front(channels=2, samples=T)
        assert lib.m17hip_set_fir_taps(ctx.h, None) == ESTATE
        assert lib.m17hip_set_fir_taps(ctx.h, cl.delta(3).ctypes.data_as(C.c_void_p)) == ESTATE
        ctx.run(channels=2, samples=T)
        ctx.frames()
        ctx.reset()
        ctx.upload(x[:1, :150])
        assert np.array_equal(_u32(ctx.fir()), _u32(cl.fir(xf[:1, :150], t)))      # ... and still
    finally:
        ctx.upload_wait()
        ctx.reset()
        ctx.set_fir_taps(None)


# ---- whole chain with a tilted RRC -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    c = m17hip.Context(cl.TILT_C, cl.TILT_T)
    c.set_fir_taps(cl.tilted_rrc())
    yield c
    c.close()


TILT_CELLS = {"default": {}, "segments_of_9600": {3: 9600}, "gate_aware": {3: 9600, 26: 1}}


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("cell", list(TILT_CELLS) + ["runs_of_9600"])
def test_full_chain_with_a_tilted_rrc(chain, cell, dtype):
    """h'[i] = fl32(h[i] (1 + 0.02 (i - 74) / 74)) demodulates as the RRC does and has no two mirrored taps equal.  32 channels x 72 000 samples, a burst,
    noise that loses the sync, a second burst (the two-burst construction of tests/test_gpu_parity.py): every channel's gate closes and reopens, which is
    where the sequential kernel's own filter and K2's patch window read the taps and the raw history.  The default schedule, segments of 9600 with and
    without the gate-aware front end (key 26 = 1), and the stream cut into runs of 9600 (carried history); int16 and float32."""
    x = cl.tilted_input()
    r = cl.tilted_oracle()
    xx = fl.on_grid(x) if dtype == "float32" else x
    keys = TILT_CELLS.get(cell, {})
    defaults = {3: 48000, 26: -1}
    for k, v in keys.items():
        chain.tune(k, v)
    try:
        cl.check_stream(chain, xx, r, 9600 if cell == "runs_of_9600" else cl.TILT_T, f"tilted RRC, {cell}, {dtype}")
    finally:
        for k in keys:
            chain.tune(k, defaults[k])


def test_taps_hold_across_a_reset_and_are_not_the_rrc(chain):
    """The taps stay in force across m17hip_demod_reset (every cell above resets first); and the tilt is seen: the RRC's records on this input differ."""
    x = cl.tilted_input()
    chain.reset()
    chain.upload(x)
    chain.run()
    got = chain.frames()
    assert got.tobytes() == cl.tilted_oracle().frames().tobytes()
    recs, counts, _ = ol.demod_batch(x, cap=cl.tilted_oracle().recs.shape[1], threads=16)
    assert got.tobytes() != np.concatenate([recs[c, :counts[c]] for c in range(x.shape[0])]).tobytes()
