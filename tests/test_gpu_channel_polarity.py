"""GPU tests of m17hip_set_channel_polarity (include/m17hip.h): the reference's -i per channel of one context.  The effective polarity of channel c
in a call is table[c] XOR the call's M17HIP_FLAG_INVERT, in the matched filter (K1), the carrier detect (K3, both forms), the limit-filter replay's
and the sequential kernel's own rescaling, and a channel whose entry changes after it has run starts over as m17hip_demod_reset_channels starts it.
Every comparison is exact: float tables as uint32 words, records and m17_diag byte for byte, against the oracle run per channel under that
channel's polarity."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import m17hip
import oracle_lib as ol

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
THREADS = 16
INV = m17hip.FLAG_INVERT
INT_FIELDS = ("dcd", "locked", "sample_index", "viterbi_cost", "n_diag", "demod_state", "n_frames")
FLOAT_FIELDS = ("evm", "deviation", "offset", "clock")


def _call(ctx, table):
    """The C entry itself: its return code."""
    if table is None:
        return ctx.lib.m17hip_set_channel_polarity(ctx.h, None, C.c_uint32(0))
    t = np.ascontiguousarray(table, dtype=np.uint8)
    return ctx.lib.m17hip_set_channel_polarity(ctx.h, t.ctypes.data_as(C.c_void_p), C.c_uint32(t.size))


def _bits(s):
    return np.array([int(ch) for ch in s], dtype=np.uint8)


# ---- 1: K1, polarity per (channel, tile) item ----------------------------------------------------------------------------------------------
FIR_C, FIR_T = 5, 2 * 4096 + 37   # three tiles per channel, the last one ragged


@pytest.fixture(scope="module")
def fir_case():
    rng = np.random.default_rng(604)
    x = rng.integers(-32768, 32768, size=(FIR_C, FIR_T), dtype=np.int64).astype(np.int16)
    x[:, 3::61] = -32768
    x[:, 7::53] = 32767
    exp = np.stack([np.stack([ol.fir_i16(x[c], invert=inv) for c in range(FIR_C)]) for inv in (0, 1)])
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


@pytest.mark.parametrize("grid", [1, 2])
def test_matched_filter_applies_the_polarity_of_the_item_it_stages(fir_case, grid):
    """m17hip_tune key 13 = 1 / 2 workgroups: one workgroup walks items of alternating polarity in a row, the next item's input in flight meanwhile."""
    x, exp = fir_case
    assert not np.array_equal(exp[0].view(np.uint32), exp[1].view(np.uint32))
    ctx = m17hip.Context(FIR_C, FIR_T)
    try:
        ctx.tune(13, grid)
        ctx.upload(x)
        for pat in ("01010", "00111", "10000"):
            pol = _bits(pat)
            ctx.set_channel_polarity(pol)
            for flag in (0, INV):
                y = ctx.fir(flags=flag)
                for c in range(FIR_C):
                    e = exp[pol[c] ^ (1 if flag else 0), c]
                    assert np.array_equal(y[c].view(np.uint32), e.view(np.uint32)), (pat, flag, c, int(np.flatnonzero(y[c].view(np.uint32) != e.view(np.uint32))[0]))
    finally:
        ctx.close()


# ---- 2: K3, both forms, polarity per lane pair ---------------------------------------------------------------------------------------------
DCD_CMAX, DCD_TMAX = 65, 1000


@pytest.fixture(scope="module")
def table_case():
    """Full-range input with -32768 in every channel in every tick (the one sample whose negation is not its opposite: without it the two tables
    of a channel are identical); the oracle's sums for every cell under both polarities."""
    rng = np.random.default_rng(20261017)
    x = rng.integers(-32768, 32768, size=(DCD_CMAX, DCD_TMAX), dtype=np.int64).astype(np.int16)
    x[:, 5::97] = -32768
    x[:, 11::89] = 32767
    ticks = DCD_TMAX // 192
    exp = np.zeros((2, DCD_CMAX, ticks, 2, 6), dtype=np.float32)
    for inv in (0, 1):
        for c in range(DCD_CMAX):
            xs = ol.scale(x[c], invert=inv)
            for k in range(ticks):
                for j in range(6):
                    a0 = 0 if j == 5 else max(k - ((k - j) % 5), 0)   # sum j restarts with the ticks = j (mod 5); sum 5 runs from the stream start
                    exp[inv, c, k, :, j] = ol.dcd_sums(xs, 192 * a0, 192 * (k - a0 + 1))
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


def _dcd_patterns(Cn):
    rng = np.random.default_rng(17 + Cn)
    return {"alternating": (np.arange(Cn) & 1).astype(np.uint8), "first_32_plain": (np.arange(Cn) >= 32).astype(np.uint8),
            "random": rng.integers(0, 2, Cn).astype(np.uint8)}


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("Cn", [1, 33, 65])
def test_carrier_detect_table_per_channel_polarity(table_case, Cn, form):
    x, exp = table_case
    diff = (exp[0].view(np.uint32) != exp[1].view(np.uint32)).reshape(DCD_CMAX, DCD_TMAX // 192, -1).any(axis=2)
    assert diff.all(), "the oracle's two tables of a channel must differ in every tick, or the case proves nothing"
    ctx = m17hip.Context(DCD_CMAX, DCD_TMAX)
    try:
        ctx.tune(10, form)
        for name, pol in _dcd_patterns(Cn).items():
            ctx.set_channel_polarity(pol)
            for T in (31, 192, 193, 960, 1000):   # (960: the four-wave form past the first lap of its producer's prefetch slots)
                ctx.upload(x[:Cn, :T])
                for flag in (0, INV):
                    sums = ctx.dcd(flags=flag)
                    eff = pol ^ (1 if flag else 0)
                    e = np.stack([exp[eff[c], c, : T // 192] for c in range(Cn)])
                    assert sums.shape == e.shape
                    bad = np.flatnonzero((sums.view(np.uint32) != e.view(np.uint32)).reshape(Cn, -1).any(axis=1))
                    assert bad.size == 0, (name, T, flag, bad[:16].tolist())
    finally:
        ctx.close()


# ---- the full chain: expectations per run, per channel under its polarity and from its latest restart --------------------------------------
def _expect(x, T, pols, restarts=None, logs=False):
    """pols[r][c]: channel c's effective polarity in run r; restarts: {run: channels that start over there}.  Per run: the oracle's records of
    that run per channel, m17_diag at its end, and (logs) the run's diagnostic callbacks — each channel demodulated by a fresh oracle from its
    latest restart to the end of the run, under its polarity."""
    Cn, n_runs = x.shape[0], len(pols)
    org = np.zeros(Cn, dtype=np.int64)
    out = []
    for r in range(n_runs):
        for c in (restarts or {}).get(r, ()):
            org[c] = r
        rows, diags, lg = [None] * Cn, np.zeros(Cn, dtype=ol.DIAG), [None] * Cn
        for a in np.unique(org):
            for inv in (0, 1):
                chs = np.flatnonzero((org == a) & (np.asarray(pols[r]) == inv))
                if not chs.size:
                    continue
                seg = np.ascontiguousarray(x[chs, a * T:(r + 1) * T])
                recs, counts, d = ol.demod_batch(seg, invert=inv, cap=2 * (seg.shape[1] // 1920 + 2) + 4, threads=THREADS)
                first = (r - a) * T
                for i, c in enumerate(chs):
                    rc = recs[i, : counts[i]]
                    rc = rc[rc["sample_pos"] >= first].copy()
                    rc["channel"] = c
                    rows[c] = rc
                    diags[c] = d[i]
                    if logs:
                        full = ol.demod_diag_log(seg[i], invert=inv, cap=seg.shape[1] // 384 + 2)
                        pos = full["pad"][:, 0].astype(np.uint64) | (full["pad"][:, 1].astype(np.uint64) << np.uint64(32))
                        lg[c] = full[pos >= first].copy()
        out.append((rows, diags, lg))
    return out


def _assert_run(got, d, exp, what, glog=None):
    rows, diags, lg = exp
    e = np.concatenate(rows)
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


# ---- 3: a uniform table and the flag are the same thing ------------------------------------------------------------------------------------
def test_all_ones_table_equals_the_invert_flag(fir_case, table_case):
    Cn, T = 8, 24000
    p = ol.gen_params(seed=1234, kind=-1, n_frames=9, lead_in=3072, noise_sigma=400.0, tail_sigma=400.0, lead_sigma=40000.0, total=T)
    xc = ol.generate_batch(p, Cn, T, threads=4)
    ctx = m17hip.Context(max(Cn, FIR_C), T)

    def everything(flag):
        out = []
        ctx.reset()   # (the operators read the input prefix a run leaves behind: the same zero history for every pass)
        ctx.upload(fir_case[0]); out.append(ctx.fir(flags=flag).tobytes())
        ctx.upload(table_case[0][:FIR_C]); out.append(ctx.dcd(flags=flag).tobytes())
        ctx.upload(xc); ctx.reset(); ctx.run(flags=flag)
        out.append(ctx.frames().tobytes()); out.append(ctx.diag(Cn).tobytes())
        return out
    try:
        plain, flagged = everything(0), everything(INV)
        assert plain[2] != flagged[2] and len(plain[2]) > 0
        ctx.set_channel_polarity(np.ones(max(Cn, FIR_C), dtype=np.uint8))
        assert everything(0) == flagged
        assert everything(INV) == plain
        ctx.set_channel_polarity(None)
        assert everything(0) == plain
    finally:
        ctx.close()


# ---- 4: the full chain under a mixed table -------------------------------------------------------------------------------------------------
CH_C, CH_T = 64, 96000


@pytest.fixture(scope="module")
def chain_case():
    """Rows from two generations of the same seed, plain and inverted transmitters, picked by a random pattern; the table is that pattern."""
    kw = dict(seed=6040, kind=-1, n_frames=CH_T // 1920 - 6, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=CH_T)
    x0 = ol.generate_batch(ol.gen_params(invert=0, **kw), CH_C, CH_T, threads=THREADS)
    x1 = ol.generate_batch(ol.gen_params(invert=1, **kw), CH_C, CH_T, threads=THREADS)
    pol = np.random.default_rng(64).integers(0, 2, CH_C).astype(np.uint8)
    assert 16 < pol.sum() < 48
    x = np.where(pol[:, None] == 1, x1, x0)
    whole = _expect(x, CH_T, [pol])[0]
    wrong = _expect(x, CH_T, [pol ^ 1])[0]
    assert all(r.size > 6 for r in whole[0]), "every channel yields frames under its right polarity"
    # Under the wrong polarity an inverted transmitter yields none of ITS frames.  (Not "no records at all": the reference demodulator, fed the negated
    # signal, takes some inverted sync words for others and reports a few BERT / LICH records of its own making — about half the count at most here.
    # What the case needs is that the polarity decides what a channel reports.)
    for c in np.flatnonzero(pol):
        right, other = whole[0][c], wrong[0][c]
        assert other.size < right.size, (c, other.size, right.size)
        keys = lambda r: {(int(q["sample_pos"]), q["payload"].tobytes()) for q in r}
        assert not keys(other) & keys(right), c
    x.setflags(write=False)
    return x, pol, whole


@pytest.mark.parametrize("knobs", [{}, {3: 4800}, {26: 1}, {20: 1}, {15: 0, 17: 0}], ids=["default", "seg4800", "gate_aware", "redo_in_front", "decode_and_evm_in_k5"])
def test_full_chain_mixed_polarity(chain_case, knobs):
    x, pol, whole = chain_case
    ctx = m17hip.Context(CH_C, CH_T)
    try:
        for k, v in knobs.items():
            ctx.tune(k, v)
        ctx.set_channel_polarity(pol)
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        _assert_run(ctx.frames().copy(), ctx.diag(CH_C), whole, str(knobs))
    finally:
        ctx.close()


def test_full_chain_mixed_polarity_staged_live_feed(chain_case):
    import torch
    x, pol, _ = chain_case
    n_runs, T = 3, CH_T // 3
    exp = _expect(x, T, [pol] * n_runs)
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(n_runs)]
    ctx = m17hip.Context(CH_C, T)
    try:
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), CH_C, T)
        ctx.run(channels=CH_C, samples=T)
        for r in range(n_runs):
            d = None
            if r + 1 < n_runs:
                ctx.upload_async(pins[r + 1].data_ptr(), CH_C, T)
                ctx.front(channels=CH_C, samples=T)
                ctx.run(channels=CH_C, samples=T)
                ctx.frames_select(1)
            else:
                d = ctx.diag(CH_C)
            got = ctx.frames().copy()
            ctx.frames_select(0)
            _assert_run(got, d, exp[r], f"live feed, run {r}")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 5: the rescaling K5 and the replay do themselves --------------------------------------------------------------------------------------
def test_dropped_channels_rescale_under_their_own_polarity():
    """Short transmissions between loud, quiet and no noise (tests/test_gpu_long_runs.py's bursty input, shortened): channels leave the limit-filter
    replay and both kernels rebuild windows from the int16 input.  Every fourth channel transmits inverted, and the table says so."""
    Cn, T = 33, 240000
    rng = np.random.default_rng(5150)
    x = np.zeros((Cn, T), dtype=np.int16)
    pol = (np.arange(Cn) % 4 == 3).astype(np.uint8)
    for c in range(Cn):
        pos = 0
        while pos < T - 9000:
            n = min(int(rng.integers(9000, 70000)), T - pos)
            p = ol.gen_params(seed=int(rng.integers(1, 1 << 30)), kind=int(rng.choice([0, 1, 2, 4])), n_frames=int(rng.integers(1, 9)),
                              lead_in=int(rng.integers(0, 6000)), lead_sigma=float(rng.choice([100.0, 20000.0, 40000.0])),
                              noise_sigma=float(rng.choice([100.0, 600.0, 1500.0])), tail_sigma=float(rng.choice([100.0, 5000.0, 20000.0])),
                              phase=int(rng.integers(-1, 10)), invert=int(pol[c]), total=n)
            x[c, pos:pos + n] = ol.generate(p)[:n]
            pos += n
        x[c, pos:] = rng.integers(-300, 300, T - pos)
    exp = _expect(x, T, [pol], logs=True)[0]
    assert sum(r.size for r in exp[0]) > Cn
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.tune(3, 4800)
        ctx.tune(9, T // 384 + 2)
        ctx.set_channel_polarity(pol)
        ctx.upload(x)
        ctx.reset()
        ctx.run()
        got, d, log = ctx.frames().copy(), ctx.diag(Cn), ctx.diag_log(Cn, capacity=T // 384 + 2)
        assert ctx.replay_drops() > 0
        _assert_run(got, d, exp, "bursty", glog=log)
    finally:
        ctx.close()


# ---- 6: a change between runs ---------------------------------------------------------------------------------------------------------------
def _stream8(T, n_runs, seed):
    p = ol.gen_params(seed=seed, kind=-1, n_frames=(n_runs * T) // 1920 - 4, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=n_runs * T)
    return ol.generate_batch(p, 8, n_runs * T, threads=8)


def test_a_changed_channel_starts_over_under_its_new_polarity():
    Cn, T, n_runs = 8, 19200, 3
    x = _stream8(T, n_runs, seed=6046).copy()
    x[[2, 5]] = np.where(np.arange(n_runs * T) >= T, -x[[2, 5]], x[[2, 5]])   # receivers 2 and 5 change sides after the first run
    pol0 = np.zeros(Cn, dtype=np.uint8)
    pol1 = pol0.copy(); pol1[[2, 5]] = 1
    exp = _expect(x, T, [pol0, pol1, pol1], restarts={1: [2, 5]})
    for c in (2, 5):   # (on the oracle alone) the restarted channels report again, counted from their restart
        later = np.concatenate([exp[1][0][c], exp[2][0][c]])
        assert later.size > 2 and later["seq"][0] == 0 and later["sample_pos"][0] < 2 * T
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.reset()
        ctx.upload(x[:, :T]); ctx.run()
        ctx.set_channel_polarity(pol1)
        ctx.upload(x[:, T:2 * T]); ctx.run()
        ctx.frames_select(1)
        _assert_run(ctx.frames().copy(), None, exp[0], "run 0, fetched after run 1 was queued")
        ctx.frames_select(0)
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[1], "run 1")
        ctx.upload(x[:, 2 * T:]); ctx.run()
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[2], "run 2")
    finally:
        ctx.close()


def test_a_change_off_the_tick_grid_is_refused_and_leaves_the_table():
    Cn, T = 8, 19200
    x = _stream8(T, 2, seed=6047)[:, : 2 * T]
    pol = _bits("01000010")
    cuts = [0, T + 1, 2 * T]
    whole = _expect(x, 2 * T, [pol])[0]
    ctx = m17hip.Context(Cn, T + 1)
    try:
        ctx.set_channel_polarity(pol)
        ctx.reset()
        ctx.upload(x[:, : T + 1]); ctx.run()
        first = ctx.frames().copy()
        flipped = pol.copy(); flipped[[2, 5]] ^= 1
        assert _call(ctx, flipped) == ESTATE
        assert _call(ctx, pol) == 0            # the values the entries have: nothing to restart, wherever the stream stands
        assert _call(ctx, pol[:3]) == 0
        ctx.upload(x[:, T + 1:]); ctx.run()
        got = np.concatenate([first, ctx.frames().copy()])
        got = got[np.lexsort((got["seq"], got["channel"]))]
        assert got.tobytes() == np.concatenate(whole[0]).tobytes(), "the stream went on under the old table, nothing was restarted"
        d = ctx.diag(Cn)
        for f in INT_FIELDS:
            assert np.array_equal(d[f], whole[1][f]), f
    finally:
        ctx.close()


# ---- 7: a table set while a run is in flight ------------------------------------------------------------------------------------------------
def test_a_run_in_flight_keeps_the_table_it_was_queued_with():
    import torch
    Cn, T = 8, 19200
    x = _stream8(T, 2, seed=6048)
    old, new = _bits("01100000"), _bits("00101001")
    changed = np.flatnonzero(old != new).tolist()
    exp = _expect(x, T, [old, new], restarts={1: changed})
    assert sum(r.size for r in exp[0][0]) > 0 and sum(r.size for r in exp[1][0]) > 0
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(2)]
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.set_channel_polarity(old)
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), Cn, T)
        ctx.run(channels=Cn, samples=T)
        ctx.set_channel_polarity(new)           # at once: run 0 is in flight
        ctx.upload_async(pins[1].data_ptr(), Cn, T)
        ctx.run(channels=Cn, samples=T)
        ctx.frames_select(1)
        _assert_run(ctx.frames().copy(), None, exp[0], "run 0 under the old table")
        ctx.frames_select(0)
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[1], "run 1 under the new table")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 7b: a device copy written again after a run has read it --------------------------------------------------------------------------------
RE_T, RE_RUNS, RE_SEED = 19200, 5, 6051
RE_FLIPS = {1: [2, 5], 2: [0], 3: [5, 7], 4: [3]}   # run: the receivers that change sides in front of it


@pytest.fixture(scope="module")
def reuse_case():
    """Five runs, a different table in front of each of runs 1 to 4, the changed channels' input negated from that run on: four tables and four reset
    lists go up, so each of the two device copies of either is written a second time after a run has read it."""
    Cn, T = 8, RE_T
    x = _stream8(T, RE_RUNS, seed=RE_SEED).copy()
    pols = [np.zeros(Cn, dtype=np.uint8)]
    for r in range(1, RE_RUNS):
        pol = pols[-1].copy()
        pol[RE_FLIPS[r]] ^= 1
        assert 0 < pol.sum() < Cn, "a mixed table: only that one is put on the device"
        pols.append(pol)
        x[RE_FLIPS[r], r * T:] = -x[RE_FLIPS[r], r * T:]
    exp = _expect(x, T, pols, restarts=RE_FLIPS)
    for r in range(RE_RUNS):   # (on the oracle alone)
        assert sum(rows.size for rows in exp[r][0]) > 0, r
    for r, chs in RE_FLIPS.items():   # a restarted channel reports again, counted from its restart, before it is restarted again or the stream ends
        for c in chs:
            end = min([q for q, cc in RE_FLIPS.items() if q > r and c in cc] + [RE_RUNS])
            later = np.concatenate([exp[q][0][c] for q in range(r, end)])
            assert later.size > 0 and later["seq"][0] == 0 and 0 < later["sample_pos"][0] <= (end - r) * T, (r, c)
    x.setflags(write=False)
    return x, pols, exp


def test_copies_written_again_after_a_run_has_read_them_in_place(reuse_case):
    x, pols, exp = reuse_case
    Cn, T = 8, RE_T
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.reset()
        for r in range(RE_RUNS):
            if r:
                ctx.set_channel_polarity(pols[r])
            ctx.upload(x[:, r * T:(r + 1) * T]); ctx.run()
            _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[r], f"in place, run {r}")
    finally:
        ctx.close()


def test_copies_written_again_after_a_run_has_read_them_staged_live_feed(reuse_case):
    import torch
    x, pols, exp = reuse_case
    Cn, T = 8, RE_T
    pins = [torch.from_numpy(np.ascontiguousarray(x[:, r * T:(r + 1) * T])).pin_memory() for r in range(RE_RUNS)]
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.reset()
        ctx.upload_async(pins[0].data_ptr(), Cn, T)
        ctx.run(channels=Cn, samples=T)
        for r in range(RE_RUNS):
            if r + 1 < RE_RUNS:
                ctx.set_channel_polarity(pols[r + 1])   # at once: run r is in flight
            d = ctx.diag(Cn)                            # (m17_diag is the latest run's: read before the next one is queued)
            if r + 1 < RE_RUNS:
                ctx.upload_async(pins[r + 1].data_ptr(), Cn, T)
                ctx.run(channels=Cn, samples=T)
                ctx.frames_select(1)
            got = ctx.frames().copy()
            ctx.frames_select(0)
            _assert_run(got, d, exp[r], f"live feed, run {r}")
        ctx.upload_wait()
    finally:
        ctx.close()


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    Cn, T = 8, 19200
    x = _stream8(T, 2, seed=6049)
    pol = _bits("00110000")
    exp = _expect(x, T, [pol, pol])
    ctx = m17hip.Context(Cn, T)
    try:
        ctx.set_channel_polarity(pol)
        assert _call(ctx, np.array([0, 2, 1], dtype=np.uint8)) == EINVAL          # an entry other than 0 / 1
        assert _call(ctx, np.zeros(Cn + 1, dtype=np.uint8)) == EINVAL             # n > max_channels
        with pytest.raises(m17hip.M17HipError):
            ctx.set_channel_polarity([])                                          # (clearing is None, not an empty table)
        assert ctx.lib.m17hip_set_channel_polarity(ctx.h, None, C.c_uint32(2)) == EINVAL
        one = np.zeros(1, dtype=np.uint8)
        assert ctx.lib.m17hip_set_channel_polarity(ctx.h, one.ctypes.data_as(C.c_void_p), C.c_uint32(0)) == EINVAL
        ctx.reset()
        ctx.upload(x[:, :T]); ctx.run()
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[0], "after the refusals of arguments")
        pin = torch.from_numpy(np.ascontiguousarray(x[:, T:])).pin_memory()
        ctx.upload_async(pin.data_ptr(), Cn, T)
        ctx.front(channels=Cn, samples=T)
        assert _call(ctx, pol ^ 1) == ESTATE                                       # between front and run
        assert _call(ctx, None) == ESTATE
        ctx.run(channels=Cn, samples=T)
        ctx.upload_wait()
        _assert_run(ctx.frames().copy(), ctx.diag(Cn), exp[1], "after the refusal between front and run")
    finally:
        ctx.close()


# ---- 9: the C++ host ------------------------------------------------------------------------------------------------------------------------
def test_cxx_host_sets_the_table(tmp_path):
    from test_channel_polarity_args import build_cxx_driver
    Cn, T = 4, 24000
    kw = dict(seed=6050, kind=-1, n_frames=9, lead_in=3072, noise_sigma=400.0, tail_sigma=400.0, lead_sigma=40000.0, total=T)
    x0 = ol.generate_batch(ol.gen_params(invert=0, **kw), Cn, T, threads=4)
    x1 = ol.generate_batch(ol.gen_params(invert=1, **kw), Cn, T, threads=4)
    pol = _bits("0110")
    x = np.where(pol[:, None] == 1, x1, x0)
    rows = _expect(x, T, [pol])[0][0]
    assert all(r.size > 0 for r in rows)
    path = os.path.join(str(tmp_path), "in.i16")
    np.ascontiguousarray(x).tofile(path)
    exe = build_cxx_driver(tmp_path)
    res = subprocess.run([exe, path, str(Cn), str(T), "0110"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    assert int(lines[0]) == sum(r.size for r in rows)
    for c in range(Cn):
        first = rows[c][0]
        assert lines[1 + c] == f"{c} {rows[c].size} " + bytes(first["payload"][: first["len"]]).hex()
