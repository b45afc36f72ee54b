"""GPU tests of the wideband signal generator (ABI 617, include/m17hip.h: m17hip_synth_wide_config, m17hip_synth_wide_channels, m17hip_synth_wide,
m17hip_synth_wide_device): wide_tx_prefix_kernel and wide_tx_mux_kernel FM-modulate the int16 input slab's rows into wide IQ streams in the caller's memory.
Every comparison is exact: the device's bytes against the HOST form of the same arithmetic (tests/cxx/wide_tx_oracle.cpp: detail/core.h's wtx_* under the
host compiler), whose own worth is asserted without a GPU in tests/test_wide_tx.py.  Then refusals and state, and a loopback: a TX context's multiplex of
m17hip_synth_tx_i16 content, received by RX contexts under the channeliser, the two-stage tuner and the resampling tuner."""
import ctypes as C

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import spliced as sp
import test_gpu_synth_tx as gtx
import tx_build as tb
import wide_tx_lib as wt

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ESTATE = -1, -2, -4
FMTS = {"i16": wt.IQ_I16, "f32": wt.IQ_F32, "u8": wt.IQ_U8}
DTYPES = {wt.IQ_I16: np.int16, wt.IQ_F32: np.complex64, wt.IQ_U8: np.uint8}
RATES = [(1, 1), (5, 1), (50, 1), (128, 3), (625, 12)]
PAD = 5   # complex samples a device row is longer than W: the pitch is not W, and what lies behind a row stays as it was


def _rows(rng, Cn, n):
    """Basebands: full-scale alternation first, then random walks and plain noise."""
    x = np.zeros((Cn, n), dtype=np.int16)
    for c in range(Cn):
        if c % 3 == 0:
            x[c] = np.where((np.arange(n) + c) % 2 == 0, -32768, 32767)
        elif c % 3 == 1:
            x[c] = np.clip(np.cumsum(rng.integers(-3000, 3001, n)), -32768, 32767)
        else:
            x[c] = rng.integers(-32768, 32768, n)
    return x


def _sentinel(S, pitch, fmt):
    import torch
    if fmt == wt.IQ_F32:
        t = torch.full((S, pitch), complex(-7.0, 9.0), dtype=torch.complex64, device="cuda")
    else:
        t = torch.full((S, pitch, 2), 77, dtype=torch.int16 if fmt == wt.IQ_I16 else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _block(ctx, x, how, fmt, S):
    """One block of the context's generator from the basebands x, by the host form of the call or into a device tensor with a pitch of W + PAD."""
    ctx.upload(x)
    if how == "host":
        return ctx.synth_wide()
    _, P, Q, _ = ctx._wide_tx
    W = x.shape[1] // Q * P
    t = _sentinel(S, W + PAD, fmt)
    ctx.synth_wide(out=t)
    a = t.cpu().numpy()
    assert a[:, W:].tobytes() == _sentinel(S, PAD, fmt).cpu().numpy().tobytes(), "nothing behind a row's W samples is written"
    return np.ascontiguousarray(a[:, :W])


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype)
    if got.tobytes() != exp.tobytes():
        g, e = got.reshape(got.shape[0], got.shape[1], -1), exp.reshape(got.shape[0], got.shape[1], -1)
        bad = np.argwhere((g.view(np.uint8) != e.view(np.uint8)).reshape(g.shape[0], g.shape[1], -1).any(axis=-1))
        raise AssertionError((what, len(bad), bad[:6].tolist(), g[tuple(bad[0])], e[tuple(bad[0])]))


def _pair(Cn, S, P, Q, fmt, table, K=None, sigma=0.0, seed=0, first=0, maxT=4096):
    """(a TX context, the host form) under one configuration and table."""
    K = wt.k_stated(P) if K is None else K
    ctx = m17hip.Context(Cn, maxT)
    ctx.synth_wide_config(S, P, Q, fmt, K, sigma, seed, first)
    mux = wt.Mux(S, P, Q, K, fmt, sigma, seed, first, channels=Cn)
    if table is not None:
        ctx.synth_wide_channels(*table)
        mux.channels(*table)
    return ctx, mux


# ---- 1: every format at every rate, three sources, ragged blocks with the carries ----------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("fmt", list(FMTS), ids=list(FMTS))
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "{}_{}".format(*r))
def test_device_bytes_are_the_host_forms(rate, fmt, how):
    """Source 0 carries two channels, source 1 one, source 2 nobody (noise alone); channel 3 has amplitude 0.  About 2500 samples a row in three ragged
    blocks — more than two tiles, cut inside tiles and inside baseband samples' spans — from a count that is not 0."""
    P, Q = rate
    f = FMTS[fmt]
    rng = np.random.default_rng(17 * P + Q)
    groups = {1: (1000, 1, 1499), 5: (199, 2, 299), 50: (19, 1, 30), 128: (7, 2, 11), 625: (1, 2, 1)}[P]
    x = _rows(rng, 4, sum(groups) * Q)
    amp = [9000.0, 1234.5, 4000.0, 0.0] if f != wt.IQ_F32 else [0.75, 1.0e-3, 2.5, 0.0]
    table = ([0, 1, 0, 1], [int(v) for v in rng.integers(-(1 << 31), 1 << 31, 4)], [int(v) for v in rng.integers(0, 1 << 32, 4)], amp)
    ctx, mux = _pair(4, 3, P, Q, f, table, sigma=300.0 if f != wt.IQ_F32 else 0.01, seed=11, first=7 * P)
    try:
        a = 0
        for i, g in enumerate(groups):
            xb = x[:, a: a + g * Q]
            a += g * Q
            _same(_block(ctx, xb, how, f, 3), mux.block(xb), (rate, fmt, how, i))
    finally:
        ctx.close()


# ---- 2: 1, 2 and 65 channels on one source --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 2, 65])
@pytest.mark.parametrize("rate", [(1, 1), (50, 1), (128, 3)], ids=lambda r: "{}_{}".format(*r))
def test_channel_counts_on_one_source(rate, Cn):
    """65 channels are more than one chunk of the list at every rate (64 at 50, 3 at 1): the chain's order goes on across chunks.  Two sources; all the
    channels on source 1."""
    P, Q = rate
    rng = np.random.default_rng(Cn * P)
    n = {1: 1100, 50: 24, 128: 27}[P]
    x = _rows(rng, Cn, n)
    table = ([1] * Cn, [int(v) for v in rng.integers(-(1 << 31), 1 << 31, Cn)], [int(v) for v in rng.integers(0, 1 << 32, Cn)],
             [float(v) for v in rng.uniform(0.5, 400.0, Cn)])
    ctx, mux = _pair(Cn, 2, P, Q, wt.IQ_F32, table, first=P)
    try:
        _same(_block(ctx, x, "device", wt.IQ_F32, 2), mux.block(x), (rate, Cn))
        _same(_block(ctx, x[::-1], "host", wt.IQ_F32, 2), mux.block(x[::-1]), (rate, Cn, "second block"))
    finally:
        ctx.close()


# ---- 3: silence, noise alone, an extreme baseband ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS), ids=list(FMTS))
@pytest.mark.parametrize("sigma", [0.0, 500.0])
def test_a_source_nobody_transmits_on(sigma, fmt):
    f = FMTS[fmt]
    x = _rows(np.random.default_rng(1), 2, 300)
    ctx, mux = _pair(2, 2, 5, 1, f, None, sigma=sigma, seed=3)   # (a fresh table: every amplitude 0)
    try:
        got = _block(ctx, x, "device", f, 2)
        _same(got, mux.block(x), (sigma, fmt))
        if sigma == 0.0:
            zero = {wt.IQ_I16: 0, wt.IQ_U8: 128}.get(f)   # (rintf(127.5) is 128)
            assert got.tobytes() == (np.zeros(got.shape, dtype=got.dtype) if zero is None else np.full(got.shape, zero, dtype=got.dtype)).tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("rate", [(1, 1), (50, 1), (625, 12)], ids=lambda r: "{}_{}".format(*r))
def test_an_extreme_baseband_wraps_the_phase(rate):
    """+-32768 alternating under M17's word and under a word of 63 random bits, which wraps theta at every step; the carries across two blocks."""
    P, Q = rate
    n = {1: 2050, 50: 42, 625: 48}[P]
    x = _rows(np.random.default_rng(2), 1, n)
    assert set(np.unique(x)) == {-32768, 32767}
    for K in (wt.k_stated(P), 0x5DEECE66D1234567):
        ctx, mux = _pair(1, 1, P, Q, wt.IQ_F32, ([0], [1 << 29], [12345], [1.0]), K=K)
        try:
            for i in range(2):
                _same(_block(ctx, x, "host", wt.IQ_F32, 1), mux.block(x), (rate, hex(K), i))
        finally:
            ctx.close()


# ---- 4: a tile's edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 1, 1023), (1, 1, 1024), (1, 1, 1025), (128, 3, 21), (128, 3, 24), (128, 3, 27), (5, 1, 1), (2000, 1, 1)],
                         ids=lambda c: "{}_{}_n{}".format(*c))
def test_rows_one_short_of_equal_to_and_one_past_a_tile(case):
    """W = 1023, 1024 and 1025 at 1 / 1; 896, 1024 and 1152 at 128 / 3 (a row is a multiple of P); one baseband sample; the largest P."""
    P, Q, n = case
    assert wt.TILE == 1024
    rng = np.random.default_rng(n)
    x = _rows(rng, 3, n)
    table = ([0, 1, 0], [int(v) for v in rng.integers(-(1 << 31), 1 << 31, 3)], [0, 1 << 31, 99], [3000.0, 20000.0, 3000.0])
    ctx, mux = _pair(3, 2, P, Q, wt.IQ_I16, table, sigma=50.0, seed=n)
    try:
        for i in range(2):
            _same(_block(ctx, x, "device", wt.IQ_I16, 2), mux.block(x), (case, i))
    finally:
        ctx.close()


# ---- 5: across 2^32 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES, ids=lambda r: "{}_{}".format(*r))
def test_a_block_that_crosses_2_to_the_32(rate):
    """first_sample = 2^32 - 3 P and a block of 6 P samples: the carrier takes the count modulo 2^32, the noise all 64 bits of it.  Where P does not divide
    2^32 (5, 50, 625) that count is no multiple of P, which the configuration refuses — asserted —, and the feed begins at the multiple of P next below it:
    the block of 6 P samples crosses 2^32 all the same."""
    P, Q = rate
    first = (1 << 32) - 3 * P
    if first % P:
        probe = m17hip.Context(1, 64)
        try:
            assert _config(probe, 1, P, Q, wt.IQ_I16, first=first) == EINVAL
        finally:
            probe.close()
        first -= first % P
    assert first % P == 0 and first < (1 << 32) < first + 6 * P
    x = _rows(np.random.default_rng(P), 2, 6 * Q)
    table = ([0, 0], [0x12345677, -0x7654321], [5, 6], [8000.0, 8000.0])
    ctx, mux = _pair(2, 1, P, Q, wt.IQ_I16, table, sigma=400.0, seed=1, first=first)
    try:
        got = _block(ctx, x, "host", wt.IQ_I16, 1)
        _same(got, mux.block(x), rate)
        assert got.shape[1] == 6 * P and mux.count == first + 6 * P > (1 << 32)
        wrong = wt.Mux(1, P, Q, wt.k_stated(P), wt.IQ_I16, 400.0, 1, first - (1 << 32) + (1 << 33), channels=2)   # (the same count modulo 2^32)
        wrong.channels(*table)
        assert wrong.block(x).tobytes() != got.tobytes()
        _same(_block(ctx, x, "device", wt.IQ_I16, 1), mux.block(x), (rate, "behind it"))
    finally:
        ctx.close()


# ---- 6: table changes, resets, a new configuration -----------------------------------------------------------------------------------------------------------
def test_table_changes_resets_and_configurations():
    P, Q, f = 50, 1, wt.IQ_I16
    rng = np.random.default_rng(6)
    x = _rows(rng, 5, 40)
    t1 = ([0, 1, 0, 1, 0], [1000, -2000, 3 << 28, 77, -(1 << 31)], [0, 1, 2, 3, 4], [3000.0, 2500.0, 2000.0, 1500.0, 1000.0])
    ctx, mux = _pair(5, 2, P, Q, f, t1, sigma=20.0, seed=4, first=50 * P)
    try:
        _same(_block(ctx, x, "host", f, 2), mux.block(x), "first table")
        # two entries change between blocks: the others keep theirs, every carry goes on
        t2 = ([1, 1], [-5, 6 << 27], [9, 9], [0.0, 7000.0])
        ctx.synth_wide_channels(*t2)
        mux.channels(*t2)
        _same(_block(ctx, x[:, :17], "device", f, 2), mux.block(x[:, :17]), "second table")
        # fewer channels in a call: the table's channels past them are silent, their feeds stand still
        ctx.upload(x[:3])
        sub = wt.Mux(2, P, Q, mux.K, f, 20.0, 4, 0, channels=3)
        sub.table[:] = mux.table[:3]
        sub.a2, sub.last, sub.count = mux.a2[:3].copy(), mux.last[:3].copy(), mux.count
        _same(ctx.synth_wide(), sub.block(x[:3]), "three of five channels")
        mux.a2[:3], mux.last[:3], mux.count = sub.a2, sub.last, sub.count
        _same(_block(ctx, x, "host", f, 2), mux.block(x), "five again")
        # m17hip_demod_reset: count and carries start over, table and configuration stay
        ctx.reset()
        mux.reset()
        assert mux.count == 50 * P
        _same(_block(ctx, x, "host", f, 2), mux.block(x), "behind the reset")
        # a new configuration: a fresh table
        ctx.synth_wide_config(2, P, Q, wt.IQ_U8, mux.K, 0.0, 0, 0)
        got = _block(ctx, x, "host", wt.IQ_U8, 2)
        assert got.dtype == np.uint8 and (got == 128).all()
    finally:
        ctx.close()


# ---- 7: refusals and state ------------------------------------------------------------------------------------------------------------------------------------
def _config(ctx, S, p, q, fmt, k=1 << 40, sigma=0.0, seed=0, first=0):
    return ctx.lib.m17hip_synth_wide_config(ctx.h, C.c_uint32(S), C.c_uint32(p), C.c_uint32(q), C.c_int(fmt), C.c_uint64(k), C.c_float(sigma), C.c_uint64(seed),
                                            C.c_uint64(first))


def _channels(ctx, tx, n):
    return ctx.lib.m17hip_synth_wide_channels(ctx.h, None if tx is None else tx.ctypes.data_as(C.c_void_p), C.c_uint32(n))


def _synth(ctx, name, ptr, Cn, n, pitch):
    return getattr(ctx.lib, name)(ctx.h, None if ptr is None else C.c_void_p(ptr), C.c_uint32(Cn), C.c_uint32(n), C.c_size_t(pitch))


def test_refusals_state_memory_and_timing():
    import torch
    Cn, n, P, Q = 4, 96, 128, 3
    W = n // Q * P
    x = _rows(np.random.default_rng(8), Cn, n)
    host = np.full((2, W + PAD, 2), 77, dtype=np.int16)
    dev = _sentinel(2, W + PAD, wt.IQ_I16)
    ways = (("m17hip_synth_wide", host.ctypes.data), ("m17hip_synth_wide_device", dev.data_ptr()))
    ctx = m17hip.Context(Cn, 4096)
    try:
        tx = np.zeros(Cn, dtype=m17hip.WIDE_TX_DTYPE)
        tx["amplitude"] = 1000.0
        assert ctx.iq_bytes() == 0
        # before the configuration
        ctx.upload(x)
        assert _channels(ctx, tx, Cn) == ESTATE
        for name, ptr in ways:
            assert _synth(ctx, name, ptr, Cn, n, W + PAD) == ESTATE, name
        # the configuration's limits: nothing changes
        for bad in ((0, 5, 1), (257, 5, 1), (2, 0, 1), (2, 2001, 1), (2, 5, 0), (2, 50, 33), (2, 6, 4), (2, 128, 6), (2, 3, 5), (2, 1, 2)):
            assert _config(ctx, bad[0], bad[1], bad[2], wt.IQ_I16) == EINVAL, bad
        for fmt in (0, 4, -1):
            assert _config(ctx, 2, P, Q, fmt) == EINVAL
        for sigma in (-1.0, float("nan"), float("inf")):
            assert _config(ctx, 2, P, Q, wt.IQ_I16, sigma=sigma) == EINVAL
        assert _config(ctx, 2, P, Q, wt.IQ_I16, first=P + 1) == EINVAL
        assert _channels(ctx, tx, Cn) == ESTATE   # (still not configured)
        K = wt.k_stated(P)
        assert _config(ctx, 2, P, Q, wt.IQ_I16, k=K, sigma=10.0, seed=2, first=2 * P) == 0
        ctx._wide_tx = (2, P, Q, wt.IQ_I16)
        mux = wt.Mux(2, P, Q, K, wt.IQ_I16, 10.0, 2, 2 * P, channels=Cn)
        # the table's refusals: nothing changes
        good = tx.copy()
        good["source"] = [0, 1, 0, 1]
        good["fcw"] = [5, -5, 1 << 30, -(1 << 30)]
        assert _channels(ctx, good, Cn) == 0
        mux.channels(good["source"], good["fcw"], good["phase0"], good["amplitude"])
        for field, value in (("source", 2), ("amplitude", -1.0), ("amplitude", float("nan")), ("amplitude", float("inf"))):
            bad = good.copy()
            bad["fcw"] = 999
            bad[field][Cn - 1] = value
            assert _channels(ctx, bad, Cn) == EINVAL, (field, value)
        assert _channels(ctx, None, Cn) == EINVAL and _channels(ctx, good, Cn + 1) == EINVAL
        # the block's refusals: nothing is written, no carry moves
        for name, ptr in ways:
            assert _synth(ctx, name, None, Cn, n, W + PAD) == EINVAL
            assert _synth(ctx, name, ptr, 0, n, W + PAD) == EINVAL and _synth(ctx, name, ptr, Cn + 1, n, W + PAD) == EINVAL
            assert _synth(ctx, name, ptr, Cn, 0, W + PAD) == EINVAL and _synth(ctx, name, ptr, Cn, 4097, 1 << 20) == EINVAL
            assert _synth(ctx, name, ptr, Cn, n, W - 1) == EINVAL, "pitch < W"
            assert _synth(ctx, name, ptr, Cn - 1, n, W + PAD) == ESTATE and _synth(ctx, name, ptr, Cn, n - Q, W + PAD) == ESTATE, "not what the slab holds"
        ctx.upload(x[:, : n - 1])
        for name, ptr in ways:
            assert _synth(ctx, name, ptr, Cn, n - 1, W + PAD) == EINVAL, "samples not a multiple of q"
        # a row of more than 2^32 - 1 samples: 2000 x 2^22 (a context of 2^22 samples, nothing of that size is touched)
        big = m17hip.Context(1, 1 << 22)
        try:
            assert _config(big, 1, 2000, 1, wt.IQ_I16) == 0
            big.synth(ol.gen_params(seed=1, kind=0, n_frames=1), 1, 1 << 22)
            assert _synth(big, "m17hip_synth_wide_device", dev.data_ptr(), 1, 1 << 22, 1 << 40) == EINVAL
            assert _synth(big, "m17hip_synth_wide_device", dev.data_ptr(), 1, 1 << 22, (1 << 32) - 1) == EINVAL
        finally:
            big.close()
        # between m17hip_demod_front and its run
        ctx.upload(x)
        ctx.run()
        pin = torch.from_numpy(x.copy()).pin_memory()
        ctx.upload_async(pin.data_ptr(), Cn, n)
        ctx.front()
        for name, ptr in ways:
            assert _synth(ctx, name, ptr, Cn, n, W + PAD) == ESTATE, name
        assert _channels(ctx, good, Cn) == ESTATE and _config(ctx, 2, P, Q, wt.IQ_I16) == ESTATE
        ctx.run()
        torch.cuda.synchronize()
        assert (host == 77).all() and dev.cpu().numpy().tobytes() == host.tobytes(), "no refusal wrote anything"
        # ... and everything refused left the generator as it was: timing index 15, one entry per block
        ctx.timing(True)
        ctx.timing_reset()
        assert _synth(ctx, ways[0][0], ways[0][1], Cn, n, W + PAD) == 0
        exp = mux.block(x)
        assert host[:, :W].tobytes() == exp.tobytes() and (host[:, W:] == 77).all()
        assert _synth(ctx, ways[1][0], ways[1][1], Cn, n, W + PAD) == 0
        torch.cuda.synchronize()
        assert dev.cpu().numpy()[:, :W].tobytes() == mux.block(x).tobytes()
        ms, launches = ctx.timing_get("synth_wide")
        assert launches == 2 and ms > 0.0
        ctx.timing(False)
        # memory: the scratch plane (8 bytes per baseband sample), the carries, the host form's block, two copies of the table
        nbytes = ctx.iq_bytes()
        least = Cn * n * 8 + Cn * 8 + 2 * Cn * 4 + 2 * W * 4
        assert least <= nbytes <= least + 2 * 4 * (257 + 4 * Cn) + 4096, (nbytes, least)
        # a float stream: refused until the next reset
        ctx.reset()
        ctx.upload(x.astype(np.float32))
        for name, ptr in ways:
            assert _synth(ctx, name, ptr, Cn, n, W + PAD) == ESTATE, name
    finally:
        ctx.close()


# ---- 8: loopback on the device -----------------------------------------------------------------------------------------------------------------------------
LB_S, LB_PER = 2, 8
LB_C = LB_S * LB_PER
LB_T = 19200
LB_SEED, LB_CHAN0 = 7, 300
LB_SIGMA = 100.0
LB_A = 3900.0
LB_BINS = ((-60, -41, -8, -2, 1, 2, 33, 57), (-55, -30, -3, 0, 4, 5, 29, 60))   # channels of 12.5 kHz; 1, 2 and 4, 5 are neighbours
LB_SRC = np.repeat(np.arange(LB_S, dtype=np.uint32), LB_PER)
LB_HZ = [12500.0 * b for bins in LB_BINS for b in bins]


@pytest.fixture(scope="module")
def loopback_content():
    """2 sources x 8 channels of m17hip_synth_tx_i16 content — BERT, stream and packet transmissions in turn — on the device, and the slab the host holds."""
    assert LB_PER * LB_A + 8.0 * LB_SIGMA <= 32767.0   # (n A + 8 sigma: no sample can clip)
    transmissions = gtx.own_transmissions(617, LB_C, lambda c: 3 + c % 3)
    # The reference's demodulator acquires a transmission behind a loud lead-in or not at all, and which it is depends on the lead-in's noise and on where
    # in the stream the burst begins: the very same baseband delayed by ONE sample — which the generator does — can go from every frame decoded to none, with
    # no multiplex involved (the float oracle on the scaled baseband shows it).  Over 96 candidates (seed, chan0, timing phase), searched once on the CPU
    # with the host forms of generator and receivers, about one channel in sixteen was not acquired under one receiver or another; seed 7 at chan0 300 is a
    # candidate every receiver acquires all sixteen of.  The criterion below is the demodulator's own and is not loosened for it.
    base = ol.gen_params(seed=LB_SEED, lead_in=3072, lead_sigma=40000.0, noise_sigma=0.0, tail_sigma=100.0)
    x = tb.batch(base, transmissions, LB_T, LB_CHAN0)
    x.setflags(write=False)
    return transmissions, base, x, {}   # (and the host form's multiplex per rate, made once)


def _sent(recs, c, transmission):
    """The good records of channel c (Viterbi cost below 30, no LICH) hold the content sent: the LSF, then every row in order."""
    kind, lsf, rows = transmission
    r = recs[(recs["channel"] == c) & (recs["cost"] < 30) & (recs["frame_type"] != sp.FT_LICH)]
    n = {tb.BERT: 25, tb.STREAM: 18, tb.PACKET: 26}[kind]
    pay = r[r["frame_type"] == sp.FT_STREAM] if kind == tb.STREAM else r[r["frame_type"] != sp.FT_LSF]
    ok = [bytes(q["payload"][:n]) for q in pay][:len(rows)] == [bytes(row[:n]) for row in rows]
    if kind != tb.BERT:
        ok = ok and r.size > 0 and r[0]["frame_type"] == sp.FT_LSF and bytes(r[0]["payload"][:30]) == bytes(lsf)
    return ok


def _multiplex(content, P, Q):
    """The TX side: synth_tx on a TX context, multiplexed into a device tensor at 48000 P / Q; its bytes are the host form's."""
    transmissions, base, x, host_form = content
    tx = m17hip.Context(LB_C, LB_T)
    try:
        tx.synth_tx(base, transmissions, LB_T, LB_CHAN0)
        assert np.array_equal(tx.download(), x)
        tx.synth_wide_config(LB_S, P, Q, wt.IQ_I16, None, LB_SIGMA, 5, 0)
        fcw = [m17hip.wide_fcw(hz, P / Q) for hz in LB_HZ]
        tx.synth_wide_channels(LB_SRC, fcw, 0, LB_A)
        W = LB_T // Q * P
        t = _sentinel(LB_S, W, wt.IQ_I16)
        tx.synth_wide(out=t)
        got = t.cpu().numpy()
    finally:
        tx.close()
    if (P, Q) not in host_form:
        mux = wt.Mux(LB_S, P, Q, wt.k_stated(P), wt.IQ_I16, LB_SIGMA, 5, 0, channels=LB_C)
        mux.channels(LB_SRC, fcw, 0, LB_A)
        host_form[(P, Q)] = mux.block(x)
    _same(got, host_form[(P, Q)], ("multiplex", P, Q))
    assert int(got.max()) < 32767 and int(got.min()) > -32768, "no sample clips"
    return t, W, fcw


@pytest.mark.parametrize("rx", ["channeliser", "two_stage", "resampler"])
def test_loopback_every_channel_decodes_what_was_sent(loopback_content, rx):
    """12.5 kHz raster at 2.4 MSPS, received by the channeliser (192 bins) and by the two-stage tuner (10 x 5); the same raster at 2.048 MSPS, received by
    the resampling tuner (8, 3 / 16).  The generator delays every baseband by one sample; a demodulator finds its own symbol clock, so nothing accounts
    for it."""
    P, Q = (128, 3) if rx == "resampler" else (50, 1)
    t, W, fcw = _multiplex(loopback_content, P, Q)
    transmissions = loopback_content[0]
    ctx = m17hip.Context(LB_C, LB_T)
    try:
        if rx == "channeliser":
            ctx.wide_raster(LB_S, 50, 192)
            ctx.wide_raster_channels(LB_SRC, [m17hip.wide_bin(hz, 50, 192) for hz in LB_HZ])
        elif rx == "two_stage":
            ctx.wide_config2(LB_S, 10, 5)
            ctx.wide_channels(LB_SRC, fcw)
        else:
            ctx.wide_resample(LB_S, 8, 3, 16)
            ctx.wide_channels(LB_SRC, fcw)
        ctx.reset()
        ctx.upload_wide_device(t.data_ptr(), LB_C, LB_T, W)
        ctx.run()
        recs = ctx.frames()
    finally:
        ctx.close()
    bad = [c for c in range(LB_C) if not _sent(recs, c, transmissions[c])]
    assert not bad, (rx, bad)
