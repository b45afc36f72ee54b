"""CPU-only: the carrier scan (ABI 622, include/m17hip.h: m17hip_wide_scan, m17hip_wide_scan_fetch).  1: what the new calls promise without a GPU.  2: the
HOST form (detail/core.h's scan_peak, scan_fcw, scan_assign, scan_source under the host compiler, tests/cxx/scan_oracle.cpp) against the form STATED in
tests/scan_lib.py on crafted rows at 64 and 4096 points, word for word.  3: the open guarantee over random rows, and a feed of 12 blocks with carriers that
come and go.  4: what it is for — the 2.048 MSPS source of three transmissions tuned by a pool of four slots seeded where nobody transmits."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import scan_lib as sc
import squelch_floor_lib as sf
import squelch_lib as sq
import test_resample_input as tr
import test_wide_squelch_floor as t21

OPEN = sq.OPEN
SLOT, ASSIGNED, HELD = sc.SLOT, sc.ASSIGNED, sc.HELD
F = np.float32
SIZES = (64, 4096)


# ---- 1: exports, refusals and the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_scan", "m17hip_wide_scan_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 622
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_scan) and callable(m17hip.Context.wide_scan_fetch)
    assert m17hip.KERNELS["scan"] == 20 and m17hip.KERNELS["squelch_floor"] == 19
    assert len(set(m17hip.KERNELS.values())) == len(m17hip.KERNELS)
    assert (m17hip.SCAN_SLOT, m17hip.SCAN_ASSIGNED, m17hip.SCAN_HELD) == (SLOT, ASSIGNED, HELD)
    assert m17hip.wide_scan_guard_bins(9000.0, 2048000.0, 2048) == 9       # (9 kHz over 1 kHz bins)
    assert m17hip.wide_scan_guard_bins(9000.0, 240000.0, 4096) == 154      # (58.6 Hz bins: ceil(153.6))
    assert m17hip.wide_scan_guard_bins(9000.0, 240000.0, 64) == 3          # (3.75 kHz bins: ceil(2.4), at least 3)
    assert m17hip.wide_scan_guard_bins(1.0e6, 240000.0, 64) == 16          # (at most points / 4)
    hz = m17hip.wide_scan_hz(np.array([0, 1 << 30, -(1 << 31), -(1 << 20)], dtype=np.int32), 2048000.0)
    assert hz.dtype == np.float64 and hz.tolist() == [0.0, 512000.0, -1024000.0, -500.0]


def test_a_null_context_and_arguments_out_of_range_are_refused_and_nothing_is_written():
    lib = m17hip.load_library()
    pool = np.ones(4, dtype=np.uint8)
    for p, n, x in ((ol._p(pool), 4, 3), (None, 0, 0), (None, 4, 3), (ol._p(pool), 0, 3), (ol._p(pool), 4, 2), (ol._p(pool), 4, 0)):
        assert lib.m17hip_wide_scan(C.c_void_p(), p, C.c_uint32(n), C.c_uint32(x)) == -1, (n, x)
    fcw, flags, missed = np.full(8, 7, dtype=np.int32), np.full(8, 7, dtype=np.uint32), np.full(256, 7, dtype=np.uint32)
    n, s, j = C.c_uint32(77), C.c_uint32(78), C.c_uint32(79)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_scan_fetch(C.c_void_p(), C.c_uint32(back), ol._p(fcw), ol._p(flags), ol._p(missed), C.c_uint64(8), C.byref(n), C.byref(s),
                                          C.byref(j)) == -1
        assert lib.m17hip_wide_scan_fetch(C.c_void_p(), C.c_uint32(back), None, None, None, C.c_uint64(8), None, None, None) == -1
    assert (fcw == 7).all() and (flags == 7).all() and (missed == 7).all() and (n.value, s.value, j.value) == (77, 78, 79)


# ---- 2: the host form against the stated form on crafted rows ------------------------------------------------------------------------------------------------
def _word(k, N):
    """the bin-centre word of bin k, signed"""
    w = (k % N) << (32 - (N.bit_length() - 1))
    return w - (1 << 32) if w >= 1 << 31 else w


def _run(row, words, hold=None, J=1, B=0, X=3, lo=1.0, lc=None, med=0.0, hang=0, pool=None, n=None):
    """One source, every channel on it: the host form's (words, flags, missed), asserted equal to the stated form's."""
    row = np.asarray(row, dtype=F)
    Cn = len(words)
    floor = np.array([[med], [0.0], [lo], [lo if lc is None else lc]], dtype=F)
    args = (row[None], J, floor, B, X, hang, [0] * Cn, words, [1] * Cn if pool is None else pool, Cn if n is None else n,
            np.zeros(Cn, dtype=np.uint32) if hold is None else hold)
    got, exp = sc.block(*args), sc.block_stated(*args)
    for g, e, what in zip(got, exp, ("words", "flags", "missed")):
        assert np.array_equal(g, e), (what, g, e)
    return got[0].tolist(), got[1].tolist(), int(got[2][0])


def _peaks(band, X, to):
    band = np.asarray(band, dtype=F)
    got = sc.peaks(band, X, to)
    assert got == [k for k in range(band.size) if sc.peak_stated(band, k, X, to)]
    return got


@pytest.mark.parametrize("N", SIZES)
def test_a_flat_row_has_exactly_one_peak_bin_0(N):
    row = np.full(N, 2.0, dtype=F)
    for B in (0, 1, 4):
        band = sc.bands(row, B)
        assert np.array_equal(band.view(np.uint32), sc.bands_stated(row, B).view(np.uint32))
        assert _peaks(band, 3, 1.0) == [0] and _peaks(band, N // 4, 1.0) == [0]
        assert _peaks(band, 3, float(band[0]) * 1.5) == []
    # every slot stands on a bin over the open level: held, none free; the one held within X of bin 0 covers it
    assert _run(row, [_word(N // 2, N)] * 2) == ([_word(N // 2, N)] * 2, [SLOT | HELD] * 2, 1)
    assert _run(row, [_word(N // 2, N), _word(N - 3, N)]) == ([_word(N // 2, N), _word(N - 3, N)], [SLOT | HELD] * 2, 0)


@pytest.mark.parametrize("N", SIZES)
def test_a_plateau_across_the_wrap(N):
    row = np.zeros(N, dtype=F)
    row[[N - 3, N - 2, N - 1, 0]] = 5.0
    band = sc.bands(row, 2)
    assert band[N - 2] == band[N - 1] == 20.0 and _peaks(band, 3, 1.0) == [N - 2]       # (the tie goes to the lower index, not to the wrap's other side)
    # the centroid of bins N - 4 .. 0 over the median 0 is half a bin up: the word half way rounds to the upper bin
    w = sc.fcw(row, N - 2, 2, 0.0)
    assert w == sc.fcw_stated(row, N - 2, 2, 0.0) == _word(N - 2, N) + (1 << (31 - (N.bit_length() - 1))) and sq.bin_stated(w, N.bit_length() - 1) == N - 1
    assert _run(row, [_word(N // 2, N)], B=2) == ([w], [SLOT | ASSIGNED], 0)
    row = np.zeros(N, dtype=F)
    row[[N - 1, 0]] = 5.0
    assert _peaks(sc.bands(row, 0), 3, 1.0) == [0]                                      # (bins N - 1 and 0 tie: 0 < N - 1)


@pytest.mark.parametrize("N", SIZES)
def test_two_equal_peaks_x_apart_are_one_and_x_plus_one_apart_two(N):
    for X in (3, 5, N // 4):
        for a in (7, N - 2):
            band = np.zeros(N, dtype=F)
            band[a % N] = band[(a + X) % N] = 9.0
            assert _peaks(band, X, 1.0) == [min(a % N, (a + X) % N)], (X, a)
            band = np.zeros(N, dtype=F)
            band[a % N] = band[(a + X + 1) % N] = 9.0
            assert _peaks(band, X, 1.0) == sorted([a % N, (a + X + 1) % N]), (X, a)
            band[(a + 1) % N] = 9.5                                                     # (a stronger bin X from the second and 1 from the first beats both)
            assert _peaks(band, X, 1.0) == [(a + 1) % N], (X, a)


@pytest.mark.parametrize("N", SIZES)
def test_a_nan_and_an_inf_bin(N):
    nan, inf = F(np.nan), F(np.inf)
    band = np.zeros(N, dtype=F)
    band[10], band[11], band[30] = 9.0, nan, nan
    assert _peaks(band, 3, 1.0) == [10]                      # (a NaN neighbour beats nothing; a NaN band is no peak)
    band[12] = inf
    assert _peaks(band, 3, 1.0) == [12]
    assert _peaks(band, 3, float(inf)) == [12]
    # in a row: the bands around a NaN bin are NaNs, around an inf bin inf — the lowest of them is the peak, its centroid is not finite and counts as 0
    row = np.zeros(N, dtype=F)
    row[20], row[40] = 9.0, nan
    words, flags, missed = _run(row, [_word(N // 2, N)] * 3, B=1)
    assert words == [_word(20, N)] + [_word(N // 2, N)] * 2 and flags[0] == SLOT | ASSIGNED and missed == 0   # (band 19..21 tie: 19, a bin up by its centroid)
    row[40] = inf
    words, flags, missed = _run(row, [_word(N // 2, N)] * 3, B=1)
    assert sorted(words[:2]) == sorted([_word(39, N), _word(20, N)]) and words[0] == _word(39, N) and missed == 0
    row[21] = nan   # (beside the carrier: bands 20 .. 22 are NaNs and no peaks, bin 19 still is one, and its word lands in bin 20, whose NaN band opens)
    words, flags, missed = _run(row, [_word(N // 2, N)] * 3, B=1)
    assert words == [_word(39, N), _word(20, N), _word(N // 2, N)]
    row[19] = nan   # (on both sides: every band that holds the carrier is a NaN — no peak is left of it)
    words, flags, missed = _run(row, [_word(N // 2, N)] * 3, B=1)
    assert words == [_word(39, N)] + [_word(N // 2, N)] * 2
    assert _run(row, [_word(N // 2, N)], B=1, med=float(nan)) == ([_word(N // 2, N)], [SLOT], 0)


@pytest.mark.parametrize("N", SIZES)
def test_a_row_of_zeros(N):
    row = np.zeros(N, dtype=F)
    assert _run(row, [_word(5, N)] * 2, B=1) == ([_word(5, N)] * 2, [SLOT] * 2, 0)                    # (below the open level: no peak, no slot held)
    assert _peaks(sc.bands(row, 1), 3, 0.0) == [0]
    assert _run(row, [_word(5, N)] * 2, B=1, lo=0.0) == ([_word(5, N)] * 2, [SLOT | HELD] * 2, 1)     # (a level of +0: every bin ties at it)


@pytest.mark.parametrize("N", SIZES)
def test_a_centroid_that_lands_below_the_open_level_takes_the_bin_centre(N):
    row = np.zeros(N, dtype=F)
    k = N - 9
    row[k - 1], row[k], row[k + 1] = 1.0, 2.0, 8.0
    band = sc.bands(row, 1)
    assert (band[k], band[k + 1]) == (11.0, 10.0) and _peaks(band, 3, 10.5) == [k]
    w = sc.fcw(row, k, 1, 0.0)
    assert w == sc.fcw_stated(row, k, 1, 0.0) and sq.bin_stated(w, N.bit_length() - 1) == k + 1   # (delta = 7 / 11)
    assert sc.assign(row, band, k, 1, 0.0, 10.0) == sc.assign_stated(row, band, k, 1, 0.0, 10.0) == w
    assert sc.assign(row, band, k, 1, 0.0, 10.5) == sc.assign_stated(row, band, k, 1, 0.0, 10.5) == _word(k, N)
    assert _run(row, [0], B=1, lo=10.5) == ([_word(k, N)], [SLOT | ASSIGNED], 0)
    assert _run(row, [0], B=1, lo=10.0) == ([w], [SLOT | ASSIGNED], 0)
    assert _run(row, [0], B=1, lo=5.25, J=2) == ([_word(k, N)], [SLOT | ASSIGNED], 0)             # (the threshold is the level times the frames)


@pytest.mark.parametrize("N", SIZES)
def test_more_peaks_than_free_slots(N):
    row = np.zeros(N, dtype=F)
    at = {4: 5.0, 12: 9.0, 20: 5.0, 28: 7.0, N - 4: 5.0}
    for k, v in at.items():
        row[k] = v
    seed = _word(N // 2, N)
    # five peaks, three slots: the strongest, then the next, then the LOWEST bin of the three that tie; two are left over
    assert _run(row, [seed] * 3) == ([_word(12, N), _word(28, N), _word(4, N)], [SLOT | ASSIGNED] * 3, 2)
    # slots that are not the source's pool: a channel that is no slot, one at n or above
    assert _run(row, [seed] * 4, pool=[1, 0, 1, 1], n=3) == ([_word(12, N), seed, _word(28, N), seed], [SLOT | ASSIGNED, 0, SLOT | ASSIGNED, SLOT], 3)
    assert _run(row, [seed] * 6) == ([_word(k, N) for k in (12, 28, 4, 20, N - 4)] + [seed], [SLOT | ASSIGNED] * 5 + [SLOT], 0)


@pytest.mark.parametrize("N", SIZES)
def test_a_held_slot_covers_the_peaks_within_the_guard(N):
    for X in (3, 9):
        for p in (30, N - 2):
            row = np.zeros(N, dtype=F)
            row[p % N], row[(p + X) % N] = 5.0, 20.0          # (the slot's bin: over the close level 4, under the open level 10; the peak)
            hold = np.array([1, 0], dtype=np.uint32)
            words = [_word(p, N), _word(N // 2, N)]
            assert _run(row, words, hold=hold, X=X, lo=10.0, lc=4.0) == (words, [SLOT | HELD, SLOT], 0), (X, p)
            row = np.zeros(N, dtype=F)
            row[p % N], row[(p + X + 1) % N] = 5.0, 20.0
            assert _run(row, words, hold=hold, X=X, lo=10.0, lc=4.0) == ([words[0], _word(p + X + 1, N)], [SLOT | HELD, SLOT | ASSIGNED], 0), (X, p)
            # not open before: the same band does not hold the slot, and it is the first free one
            assert _run(row, words, X=X, lo=10.0, lc=4.0) == ([_word(p + X + 1, N), words[1]], [SLOT | ASSIGNED, SLOT], 0), (X, p)


@pytest.mark.parametrize("N", SIZES)
def test_a_slot_in_its_hang_time_is_held(N):
    row = np.zeros(N, dtype=F)
    row[33] = 20.0
    words = [_word(31, N), _word(N // 2, N)]
    assert _run(row, words, hold=np.array([2, 0], dtype=np.uint32), lo=10.0, lc=4.0, hang=3) == (words, [SLOT | HELD, SLOT], 0)
    assert _run(row, words, hold=np.array([1, 0], dtype=np.uint32), lo=10.0, lc=4.0, hang=3) == ([_word(33, N), words[1]], [SLOT | ASSIGNED, SLOT], 0)


@pytest.mark.parametrize("N", SIZES)
def test_no_frame_or_a_level_that_is_not_finite_changes_nothing(N):
    row = np.zeros(N, dtype=F)
    row[33] = 20.0
    words = [_word(5, N), _word(33, N)]
    hold = np.array([0, 3], dtype=np.uint32)
    for kw in (dict(J=0), dict(lo=float("nan")), dict(lo=float("inf")), dict(med=float("nan")), dict(med=float("-inf"))):
        assert _run(row, words, hold=hold, **kw) == (words, [SLOT, SLOT], 0), kw
    assert _run(row, words, hold=hold) == (words, [SLOT, SLOT | HELD], 0)


# ---- 3: the open guarantee, and a feed -------------------------------------------------------------------------------------------------------------------------
def _random_plane(rng, S, N, carriers, widths=(0, 1, 2)):
    p = rng.exponential(1.0, (S, N))
    for s in range(S):
        for k in rng.choice(N, carriers, replace=False):
            h = int(rng.choice(widths))
            for d in range(-h, h + 1):
                p[s, (k + d) % N] += rng.uniform(5.0, 400.0) * rng.uniform(0.2, 1.0)
    return p.astype(F)


@pytest.mark.parametrize("N", SIZES)
def test_every_slot_assigned_in_a_block_is_open_in_that_block(N):
    rng = np.random.default_rng(6220 + N)
    S, Cn = 2, 12
    src = [c % S for c in range(Cn)]
    assigned = fell_back = 0
    for trial in range(12 if N == 64 else 4):
        B, X, J, hang = int(rng.choice([0, 1, 4])), int(rng.choice([3, 5, N // 4])), int(rng.choice([1, 3, 100])), int(rng.choice([0, 2]))
        plane = (_random_plane(rng, S, N, 6) * F(J)).astype(F)
        floor = sf.Floor(S, B, F(6.0), F(3.0)).block(plane, J)
        seeds = [int(rng.integers(-(1 << 31), 1 << 31)) for _ in range(Cn)]
        squelch = sq.Squelch(src, seeds, floor[2], floor[3], B, hang)
        squelch.hold[:] = rng.integers(0, 3, Cn)
        scan = sc.Scan([1] * Cn, X, seeds)
        exp = scan.block(plane, J, floor, squelch, stated=True)
        scan.fresh = True
        words, flags, missed = scan.block(plane, J, floor, squelch)
        assert np.array_equal(words, exp[0]) and np.array_equal(flags, exp[1]) and np.array_equal(missed, exp[2]), trial
        squelch.fcw[:] = words
        state, band = squelch.block(plane, J)
        new = (flags & ASSIGNED) != 0
        assert ((state[new] & OPEN) != 0).all(), (trial, words, flags, state)
        assert (((flags & HELD) != 0) == ((state & OPEN) != 0))[~new].all()    # (and a slot is held iff the squelch finds it open on its unchanged word)
        assigned += int(new.sum())
        logn = N.bit_length() - 1
        fell_back += sum(1 for c in np.flatnonzero(new) if int(words[c]) == _word(sq.bin_stated(int(words[c]), logn), N))
    assert assigned >= 8


def test_a_feed_of_12_blocks_with_carriers_that_come_and_go():
    N, S, Cn, B, X, J, hang = 64, 2, 8, 1, 4, 10, 1
    rng = np.random.default_rng(62212)
    src = [0, 0, 0, 1, 1, 1, 0, 1]
    pool = [1, 1, 1, 1, 1, 0, 0, 0]
    seeds = [_word(k, N) for k in (2, 2, 2, 3, 3, 40, 50, 60)]
    # carrier -> (source, bin, first block, last block); the bins stand more than X apart, and bins 2 and 3 stay empty
    plan = [(0, 10, 0, 11), (0, 20, 1, 4), (0, 30, 2, 3), (0, 44, 6, 9), (0, 54, 7, 11), (1, 12, 0, 2), (1, 25, 5, 11), (1, 50, 5, 6)]
    floor, squelch, scan = sf.Floor(S, B, F(8.0), F(4.0)), sq.Squelch(src, seeds, [1.0] * S, [1.0] * S, B, hang), sc.Scan(pool, X, seeds)
    history = []
    for b in range(12):
        if b == 8:   # (a fresh start: the seeds are taken again, and the carriers still there are found again)
            floor.reset(), squelch.reset(), scan.reset()
        plane = rng.exponential(1.0, (S, N)) * J
        for s, k, first, last in plan:
            if first <= b <= last:
                plane[s, k] += 300.0 * J
        plane = plane.astype(F)
        out = floor.block(plane, J)
        squelch.open, squelch.close = out[2].copy(), out[3].copy()
        before, fresh = scan.words.copy(), scan.fresh
        exp = scan.block(plane, J, out, squelch, stated=True)
        scan.fresh = fresh
        words, flags, missed = scan.block(plane, J, out, squelch)
        assert np.array_equal(words, exp[0]) and np.array_equal(flags, exp[1]) and np.array_equal(missed, exp[2]), b
        if fresh:
            before = np.array(seeds, dtype=np.int32)
        held, new = (flags & HELD) != 0, (flags & ASSIGNED) != 0
        assert np.array_equal(words[~new], before[~new]), b                      # (a word changes by assignment alone; a held slot is never retuned)
        assert not (held & new).any() and (flags[5:] == 0).all() and np.array_equal(words[5:], seeds[5:])
        squelch.fcw[:] = words
        state, _ = squelch.block(plane, J)
        assert ((state[:5][new[:5]] & OPEN) != 0).all()
        bins = {(src[c], sq.bin_stated(int(words[c]), 6)) for c in range(5) if state[c] & OPEN}
        history.append((bins, new[:5].copy(), missed.copy()))
    for b, (bins, new, missed) in enumerate(history):
        live = [(s, k) for s, k, first, last in plan if first <= b <= last]
        per = {s: sum(1 for q in live if q[0] == s) for s in range(S)}
        slots = {0: 3, 1: 2}
        for s, k in live:   # (every carrier is tuned by an open slot within a bin, while its source has slots for it)
            if per[s] <= slots[s]:
                assert any(q[0] == s and sc.distance_stated(q[1], k, N) <= 1 for q in bins), (b, s, k, bins)
        assert missed.tolist() == [max(0, per[s] - slots[s]) for s in range(S)], (b, missed, per)
    n_new = [int(h[1].sum()) for h in history]
    assert n_new[0] == 2 and n_new[1] == 1 and n_new[2] == 1 and n_new[5] == 2 and n_new[8] == 4, n_new   # (slots reused: source 0 serves five carriers with three slots)
    assert sum(n_new) >= 11


# ---- 4: what it is for -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three():
    """The host form of the feed below, once (tests/test_gpu_wide_scan.py compares the device with it): (per block (Y, state, band, J, floor, words, flags,
    missed), seed, B, X), read-only."""
    bb, x = t21._source()
    B = m17hip.wide_squelch_half_bins(9000.0, t21.RATE, t21.POINTS)
    X = m17hip.wide_scan_guard_bins(9000.0, t21.RATE, t21.POINTS)
    seed = m17hip.wide_fcw(400000.0, tr.CH_R1 * tr.CH_D / tr.CH_U)
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    feed = sc.Feed([rl.Resampler(taps1, tr.CH_R1, tr.CH_U, tr.CH_D, taps2, seed) for _ in range(4)], [0] * 4, [x], t21.POINTS, t21.HOP)
    feed.squelch = sq.Squelch([0] * 4, [seed] * 4, [1.0], [1.0], B, t21.HANG)
    feed.floor = sf.Floor(1, B, m17hip.wide_squelch_ratio(t21.OPEN_DB), m17hip.wide_squelch_ratio(t21.CLOSE_DB))
    feed.scan = sc.Scan([1] * 4, X, [seed] * 4)
    feed.auto_reset = True   # (the caller lists the channels a block assigns in m17hip_demod_reset_channels before the block's run)
    out = []
    for a, b in t21._cuts(x.shape[0]):
        Y, P, state, band, J, floor, words, flags, missed = feed.block(a, b)
        e = (Y, state, band, J, floor, words.copy(), flags, missed)
        for v in e:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(e)
    return out, seed, B, X


def test_three_transmissions_are_tuned_in_the_block_in_which_they_appear():
    """The 2.048 MSPS source of three transmissions (-762.5, +12.5, +25 kHz), 100 ms blocks, 2048 points at hop 2048, a band of 9 kHz (B = 4), X = 9, 10 / 6 dB,
    hang 1.  Four slots, all seeded at +400 kHz where nobody transmits: exactly three assignments, all in block 0; the fourth slot closed in every block with
    a frame; every assigned offset within 900 Hz of its carrier; 7 of 7 records from each through the resampling tuner's host form and the float oracle."""
    blocks, seed, B, X = three()
    assert (B, X) == (4, 9)
    news = np.array([(e[6] & ASSIGNED) != 0 for e in blocks])
    opens = np.array([(e[1] & OPEN) != 0 for e in blocks])
    have = np.array([e[3] for e in blocks]) > 0
    assert all(e[7].tolist() == [0] for e in blocks)
    assert news[0].tolist() == [True, True, True, False] and not news[1:].any(), news
    assert opens[:, :3].all() and not opens[have][:, 3].any(), opens
    words = blocks[-1][5]
    assert int(words[3]) == seed
    hz = m17hip.wide_scan_hz(words[:3], t21.RATE)
    for target in (-762500.0, 12500.0, 25000.0):
        assert np.abs(hz - target).min() < 900.0, (target, hz)
    assert sorted(int(np.abs(hz - t).argmin()) for t in (-762500.0, 12500.0, 25000.0)) == [0, 1, 2]
    y = np.concatenate([e[0] for e in blocks], axis=1)
    for ch in range(3):
        got = fl.demod(y[ch])[0]
        assert len(tr._good(got)) == 7, hz[ch]
