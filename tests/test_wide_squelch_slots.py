"""CPU-only: the time-resolved squelch (ABI 620, include/m17hip.h: m17hip_wide_squelch_slots, m17hip_wide_squelch_slots_fetch).  1: what the new calls promise
without a GPU.  2: the slot and tile rules of detail/core.h (tests/cxx/squelch_slots_oracle.cpp under the host compiler) against a statement in Python
integers, on crafted numbers.  3: a block of one slot is ABI 619's block decision, word for word.  4: what it is for — a carrier keyed for a fifth of a block,
which the block decision misses.  5: the whole chain on an M17 transmission that begins inside a block."""
import ctypes as C
import functools

import numpy as np

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_lib as sq
import squelch_slots_lib as ssl
import test_resample_input as tr
import wide_lib as wl

OPEN = sq.OPEN
T_, F_ = True, False


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1: exports, refusals and the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_squelch_slots", "m17hip_wide_squelch_slots_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 620
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_squelch_slots) and callable(m17hip.Context.wide_squelch_slots_fetch)
    assert m17hip.KERNELS["squelch_slots"] == 18 and m17hip.KERNELS["squelch"] == 17 and len(set(m17hip.KERNELS.values())) == len(m17hip.KERNELS)


def test_a_null_context_and_arguments_out_of_range_are_refused_and_nothing_is_written():
    lib = m17hip.load_library()
    lv = np.array([2.0, 1.0], dtype=np.float32)
    for half, n, hang, lead in ((0, 0, 0, 0), (4, 1, 0, 0), (65, 1, 0, 0), (4, 1, 65536, 0), (4, 1, 0, 256), (0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFF)):
        assert lib.m17hip_wide_squelch_slots(C.c_void_p(), C.c_uint32(half), ol._p(lv) if n else None, ol._p(lv[1:]) if n else None, C.c_uint32(n),
                                             C.c_uint32(hang), C.c_uint32(lead)) == -1
    state, band, mask = np.full(8, 77, dtype=np.uint32), np.full(64, 7.0, dtype=np.float32), np.full(8, 76, dtype=np.uint32)
    n, g, t, frames = C.c_uint32(78), C.c_uint32(79), C.c_uint32(80), C.c_uint32(81)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_squelch_slots_fetch(C.c_void_p(), C.c_uint32(back), ol._p(state), ol._p(band), ol._p(mask), C.c_uint64(8), C.c_uint64(64),
                                                   C.c_uint64(8), C.byref(n), C.byref(g), C.byref(t), C.byref(frames)) == -1
        assert lib.m17hip_wide_squelch_slots_fetch(C.c_void_p(), C.c_uint32(back), None, None, None, C.c_uint64(8), C.c_uint64(64), C.c_uint64(8), None, None,
                                                   None, None) == -1
    assert (state == 77).all() and (band == 7.0).all() and (mask == 76).all() and (n.value, g.value, t.value, frames.value) == (78, 79, 80, 81)


# ---- 2: the slot and tile rules --------------------------------------------------------------------------------------------------------------------------------
def test_slots_and_their_frames():
    for J in (0, 1, 15, 16, 17, 32, 33, 1000, 1019, 1020, (1 << 24) + 5):
        G = ssl.slots(J)
        assert G == ssl.slots_stated(J), J
        for g in sorted({0, 1, G // 2, G - 2, G - 1} & set(range(G))):
            assert ssl.slot_frames(J, g) == ssl.slot_frames_stated(J, g), (J, g)
        assert sum(ssl.slot_frames_stated(J, g) for g in range(min(G, 100))) == min(J, 1600)
    assert ssl.slots(0) == 0 and ssl.slots(16) == 1 and ssl.slots(17) == 2 and ssl.slot_frames(17, 1) == 1 and ssl.slot_frames(1000, 62) == 8


def test_the_slot_of_a_sample():
    """first > 0 with samples in front of it (slot 0), the edges of every slot, a last slot of fewer than 16 frames and the samples behind the last frame
    (the last slot), and a hop whose 16-fold needs more than 32 bits with the sample index."""
    for first, hop, G in ((0, 64, 1), (37, 64, 5), (63, 64, 6), (5, 100, 3), (2047, 2048, 63), (0, 1 << 24, 4), (12345, 1 << 24, 2)):
        xs = {0, first - 1, first, first + 1, (1 << 32) - 1}
        for g in range(G + 2):
            for d in (-1, 0, 1):
                xs.add(first + 16 * hop * g + d)
        for x in sorted(v for v in xs if 0 <= v < (1 << 32)):
            assert ssl.slot_of(x, first, hop, G) == ssl.slot_of_stated(x, first, hop, G), (x, first, hop, G)
    assert ssl.slot_of(0, 37, 64, 5) == 0 and ssl.slot_of(36, 37, 64, 5) == 0 and ssl.slot_of(37 + 1023, 37, 64, 5) == 0 and ssl.slot_of(37 + 1024, 37, 64, 5) == 1
    assert ssl.slot_of(37 + 4 * 1024, 37, 64, 5) == 4 and ssl.slot_of(37 + 5 * 1024, 37, 64, 5) == 4 and ssl.slot_of(10 ** 9, 37, 64, 5) == 4


def test_the_span_of_a_tile():
    """The integer tuners (W = R T), the resampler (W = T / U * D * R1: not a multiple of T), a short last tile, and products beyond 32 bits."""
    for TO, T, W in ((255, 1020, 5100), (255, 1020, 6120), (765, 1530, 65280), (255, 33 * 255 + 7, (33 * 255 + 7) * 5), (255, 300, 1500), (765, 900, 38400),
                     (255, 1 << 20, (1 << 20) * 2560), (32 * 3, 48000, 2048000)):
        tiles = -(-T // TO)
        for t in sorted({0, 1, tiles // 2, tiles - 2, tiles - 1} & set(range(tiles))):
            assert ssl.tile_span(t, TO, T, W) == ssl.tile_span_stated(t, TO, T, W), (t, TO, T, W)
        assert ssl.tile_span(0, TO, T, W)[0] == 0 and ssl.tile_span(tiles - 1, TO, T, W)[1] == W
    assert ssl.tile_span(1, 255, 300, 1500) == (1275, 1500) and ssl.tile_span(1, 765, 1530, 65280) == (32640, 65280)
    assert ssl.tile_span(1, 96, 48000, 2048000) == (4096, 8192)


def _tile(flags, first, hop, lead, a, e):
    got = ssl.tile_open(flags, first, hop, lead, a, e)
    assert got == ssl.tile_open_stated(flags, first, hop, lead, a, e), (flags, first, hop, lead, a, e)
    return got


def test_whether_a_tile_is_open():
    hop, first = 64, 37
    S = 16 * hop
    only3 = [F_, F_, F_, T_, F_]
    # a tile inside slot 3, one inside slot 2 (open only through a lead of 1), one in slot 1 (lead 2), one in slot 4 (never: the lead looks forward)
    assert _tile(only3, first, hop, 0, first + 3 * S, first + 3 * S + 100) and not _tile(only3, first, hop, 0, first + 2 * S, first + 3 * S)
    assert _tile(only3, first, hop, 1, first + 2 * S, first + 3 * S) and not _tile(only3, first, hop, 1, first + S, first + 2 * S)
    assert _tile(only3, first, hop, 2, first + S, first + 2 * S) and not _tile(only3, first, hop, 255, first + 4 * S, first + 5 * S + 500)
    # a tile that straddles slots 2 and 3: its last sample is slot 3's first
    assert _tile(only3, first, hop, 0, first + 3 * S - 200, first + 3 * S + 1) and not _tile(only3, first, hop, 0, first + 3 * S - 200, first + 3 * S)
    # a tile longer than many slots (the resampler's): open if any of them is; a lead larger than G reaches the last slot and no further
    assert _tile(only3, first, hop, 0, 0, first + 5 * S + 99) and not _tile([F_] * 5, first, hop, 300, 0, first + 5 * S + 99)
    assert _tile([F_, F_, F_, F_, T_], first, hop, 300, 0, 10) and not _tile([F_, F_, F_, F_, T_], first, hop, 3, 0, 10)
    # the samples in front of the first frame are slot 0's, those behind the last frame the last slot's
    assert _tile([T_, F_, F_], first, hop, 0, 0, first) and not _tile([F_, T_, F_], first, hop, 0, 0, first)
    assert _tile([F_, F_, T_], first, hop, 0, first + 3 * S + 7, first + 3 * S + 60) and not _tile([F_, T_, F_], first, hop, 0, first + 3 * S + 7, first + 3 * S + 60)
    # more than 32 slots: the flags' second word
    many = [F_] * 40
    many[33] = T_
    assert _tile(many, 0, hop, 0, 33 * S, 34 * S) and not _tile(many, 0, hop, 0, 31 * S, 33 * S) and _tile(many, 0, hop, 2, 31 * S, 32 * S)
    # no frame at all: open
    assert _tile([], 0, hop, 0, 0, 50) and _tile([], 5, hop, 7, 10, 50)


def test_a_block_of_decisions_is_the_stated_one_and_the_hang_crosses_the_block_boundary():
    """Crafted rows: 2 sources of 64 bins, J = 37 (slots of 16, 16 and 5 frames), channel 0 on a bin that is loud in slot 0 alone, channel 1 on one loud in
    slot 2 alone (its last, short slot: the threshold is 5 frames'), channel 2 between close and open everywhere, channel 3 silent.  Hang 3 in slots: channel
    1 leaves the block with 4 and is open through the first three slots of the next, silent block; with J == 0 in between the count stands."""
    N, hop, first, J = 64, 64, 21, 37
    rows = np.full((2, 3, N), 1.0, dtype=np.float32)
    rows[:, 2] = 5.0 / 16.0                         # (the short slot's floor: 5 frames')
    rows[0, 0, 10] = 1000.0
    rows[1, 2, 32] = 400.0                          # (over 20 x 5 = 100, below 20 x 16: a threshold of 16 frames would miss it)
    rows[1, :, 51] = [9.0 * 16, 9.0 * 16, 9.0 * 5]  # (between close 5 and open 20 per frame)
    src, fcw = [0, 1, 1, 0], [10 << 26, -(1 << 31), -(13 << 26), 20 << 26]
    o, c = np.array([20.0, 20.0], dtype=np.float32), np.array([5.0, 5.0], dtype=np.float32)
    W, T, TO = first + 36 * hop + N + 30, 1020, 255     # (30 samples behind the last frame)
    s = ssl.SlotSquelch(src, fcw, o, c, 0, 3, 1)
    hold0 = s.hold.copy()
    state, bd, op, mask, tiles = s.block(rows, J, first, hop, TO, T, W)
    st2, bd2, op2, tl2 = s.block_stated(rows, J, first, hop, TO, T, W, hold0)
    assert tiles == 4 and np.array_equal(state, st2) and np.array_equal(_u32(bd), _u32(bd2)) and np.array_equal(op, op2)
    assert np.array_equal(ssl.unpack(mask, tiles), tl2)
    assert op.tolist() == [[T_, T_, T_], [F_, F_, T_], [F_, F_, F_], [F_, F_, F_]]
    assert state.tolist() == [2 | OPEN, 4 | OPEN, 0, 0] and s.hold.tolist() == [2, 4, 0, 0]
    # tiles of 255 outputs span 604.75 samples, slots end at 21 + 1024 and 21 + 2048.  Channel 1: slot 2 opens tile 3 (inside), tile 2 (samples 1209..1813:
    # slot 1 alone, open through the lead), tile 1 (it ends in slot 1) and not tile 0 (slot 0 + lead 1 = slot 1)
    assert ssl.unpack(mask, tiles).tolist() == [[T_] * 4, [F_, T_, T_, T_], [F_] * 4, [F_] * 4]
    # a block without a frame in between: open, the counts stand
    state, bd, op, mask, tiles = s.block(np.zeros((2, 0, N), dtype=np.float32), 0, 0, hop, TO, 10, 50)
    assert state.tolist() == [2 | OPEN, 4 | OPEN, OPEN, OPEN] and s.hold.tolist() == [2, 4, 0, 0] and mask.tolist() == [[1]] * 4 and bd.shape == (4, 0)
    # the silent block behind it: channel 1's hang runs out after three slots, and its tiles follow
    hold0 = s.hold.copy()
    quiet = np.full((2, 5, N), 1.0, dtype=np.float32)
    state, bd, op, mask, tiles = s.block(quiet, 80, 0, hop, TO, 1020, 5120)
    st2, bd2, op2, tl2 = s.block_stated(quiet, 80, 0, hop, TO, 1020, 5120, hold0)
    assert np.array_equal(state, st2) and np.array_equal(op, op2) and np.array_equal(ssl.unpack(mask, tiles), tl2)
    assert op.tolist() == [[T_, F_, F_, F_, F_], [T_, T_, T_, F_, F_], [F_] * 5, [F_] * 5] and state.tolist() == [0, 0, 0, 0]
    assert ssl.unpack(mask, tiles).tolist() == [[T_, F_, F_, F_], [T_, T_, T_, F_], [F_] * 4, [F_] * 4]   # (tile 2 spans 2560..3839: slots 2 and 3)


# ---- 3: one slot is ABI 619's block --------------------------------------------------------------------------------------------------------------------------
def test_a_block_of_one_slot_at_lead_0_is_the_block_decision_word_for_word():
    """wide_config(2, 5) on 64 points at hop 64: blocks of 200 outputs are 1000 samples, 15 frames or 14 as `first` varies — one slot, one tile.  The slot form
    at lead 0 and squelch_lib's block form, from the same levels and hang: state words, bands and slabs."""
    rng = np.random.default_rng(6200)
    Wb, nb = 1000, 5
    n = np.arange(nb * Wb)
    x = 20.0 * (rng.standard_normal((2, n.size)) + 1j * rng.standard_normal((2, n.size)))
    words = [10 << 26, -(1 << 31), 20 << 26]
    x[0] += np.repeat([5000.0, 0.0, 0.0, 5000.0, 0.0], Wb) * np.exp(2j * np.pi * ((words[0] * n) % (1 << 32)) / float(1 << 32))
    x[1] += np.repeat([0.0, 5000.0, 33.0, 0.0, 0.0], Wb) * np.exp(2j * np.pi * ((words[1] * n) % (1 << 32)) / float(1 << 32))
    data = np.clip(np.rint(np.stack([x.real, x.imag], axis=-1)), -32768, 32767).astype(np.int16)
    src, fcw = [0, 1, 1], words
    noise = np.clip(np.rint(20.0 * rng.standard_normal((Wb, 2))), -32768, 32767).astype(np.int16)
    p0, J0, _ = spl.plane(noise, 64, 64)
    o, c = m17hip.wide_squelch_levels(np.stack([p0, p0]), J0, 1, 20.0, 10.0)
    taps = m17hip.wide_default_taps(5)
    a = sq.Feed([wl.Tuner(taps, 5, w, 5.0 / 3.0) for w in fcw], src, data, 64, 64)
    a.squelch = sq.Squelch(src, fcw, o, c, 1, 1)
    b = ssl.Feed([wl.Tuner(taps, 5, w, 5.0 / 3.0) for w in fcw], src, data, 64, 64, ssl.WIDE_TILE)
    b.squelch = ssl.SlotSquelch(src, fcw, o, c, 1, 1, 0)
    opens = []
    for k in range(nb):
        Ya, Pa, state, band, J = a.block(k * Wb, (k + 1) * Wb)
        Yb, Pb, Ub, dec = b.block(k * Wb, (k + 1) * Wb)
        assert J == dec[5] and 1 <= J <= 16 and dec[1].shape == (3, 1) and dec[4] == 1
        assert np.array_equal(state, dec[0]) and np.array_equal(_u32(band), _u32(dec[1][:, 0])), k
        assert np.array_equal(dec[3][:, 0], (state >> 31).astype(np.uint32))
        assert np.array_equal(_u32(Ya), _u32(Yb)) and np.array_equal(_u32(Pa), _u32(Pb)), k
        opens.append(((state & OPEN) != 0).astype(int).tolist())
    assert opens == [[1, 0, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0]], opens   # (both forms open, hold on the weak tone, hang one block and close)


# ---- 4: dilution -----------------------------------------------------------------------------------------------------------------------------------------------
POINTS, HOP, RATE = 2048, 2048, 2048000.0
OPEN_DB, CLOSE_DB = 10.0, 6.0


def _band_per_frame(plane, J, k, B):
    return float(sq.band_stated(plane, k, B)) / J


def test_a_carrier_keyed_for_a_fifth_of_a_block_is_missed_by_the_block_decision_and_kept_by_the_slots():
    """One 2.048 MSPS float32 source of low noise, one block of 1 s (1000 frames of 2048 points at hop 2048, 63 slots, the last of 8 frames), open 10 dB and
    close 6 dB over the median floor.  A carrier whose band power per frame is 12 dB over the floor is keyed from 400 to 600 ms.  ABI 619's block decision:
    closed — 1 + 0.2 x 14.8 is 6 dB.  The slot form at lead 1 and hang 1: the tiles over the carrier are open, the tile in front of the first carried slot
    too, and the tiles beyond lead and hang are closed; a channel on empty spectrum has no open tile."""
    rng = np.random.default_rng(6201)
    W = 2048000
    f_c, f_e = 300000.0, -450000.0
    B = m17hip.wide_squelch_half_bins(9000.0, RATE, POINTS)
    fcw = [m17hip.wide_fcw(f_c, 128.0 / 3.0), m17hip.wide_fcw(f_e, 128.0 / 3.0)]
    k_c = sq.bin_stated(fcw[0], 11)
    noise = (rng.standard_normal((W, 2)) * 10.0).astype(np.float32)
    n = np.arange(W)
    tone = np.exp(2j * np.pi * ((fcw[0] * n) % (1 << 32)) / float(1 << 32))
    # the floor of the band per frame, and the band per frame of the tone at amplitude 1: the amplitude that puts the keyed band at 10^1.2 floors
    p_n, J, _ = spl.plane(noise.view(np.complex64).reshape(-1), POINTS, HOP)
    assert J == 1000
    o, c = m17hip.wide_squelch_levels(p_n[None, :], J, B, OPEN_DB, CLOSE_DB)
    floor = float(np.median(p_n.astype(np.float64))) * (2 * B + 1) / J
    p_t, Jt, _ = spl.plane(tone[:16 * HOP].astype(np.complex64), POINTS, HOP)
    ampl = np.sqrt((10.0 ** 1.2 - 1.0) * floor / _band_per_frame(p_t, Jt, k_c, B))
    a0, a1 = 819200 + 5000, 819200 + 5000 + 409600          # (200 ms from 402.4 ms: neither edge on a slot's)
    x = noise.view(np.complex64).reshape(-1).astype(np.complex128)
    x[a0:a1] += ampl * tone[a0:a1]
    row = x.astype(np.complex64)
    # the premise: per frame the keyed band is 12 dB over the floor (within half a dB: the noise's cross terms), and the block's is 6 dB — closed under ABI 619
    keyed, Jk, _ = spl.plane(row[a0 - a0 % HOP + HOP: a0 - a0 % HOP + 17 * HOP], POINTS, HOP)
    assert abs(10.0 * np.log10(_band_per_frame(keyed, Jk, k_c, B) / floor) - 12.0) < 0.5
    plane, J, first = spl.plane(row, POINTS, HOP)
    assert (J, first) == (1000, 0) and abs(10.0 * np.log10(_band_per_frame(plane, J, k_c, B) / floor) - 6.0) < 0.5
    blk = sq.Squelch([0, 0], fcw, o, c, B, 0)
    state, band = blk.block(plane[None, :], J)
    assert state.tolist() == [0, 0], "the block decision hears the diluted carrier: the premise of this test is gone"
    # the slot form under the resampler's tile at 16 x 3 / 8 ... here 8 x 3 / 16, 48 000 outputs
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    TO = rl.tile_outputs(taps1.size, tr.CH_R1, taps2.size, tr.CH_U, tr.CH_D)
    rows, J2, first2 = ssl.slot_rows(row, POINTS, HOP)
    assert (J2, first2) == (J, first) and rows.shape == (63, POINTS)
    two, _, _ = spl.plane(row[: 32 * HOP], POINTS, HOP)      # (the slots' rows are the spectrum's first-level sums: two of them add to a plane of 32 frames)
    assert np.array_equal(_u32(two), _u32(np.float32(np.float32(0.0) + rows[0]) + rows[1]))
    s = ssl.SlotSquelch([0, 0], fcw, o, c, B, 1, 1)
    state, bd, op, mask, tiles = s.block(rows[None], J, first, HOP, TO, 48000, W)
    S = 16 * HOP
    g0, g1 = -(-a0 // S), a1 // S - 1                         # the slots wholly under the carrier
    assert op[0, g0:g1 + 1].all() and not op[0, : a0 // S].any() and not op[0, a1 // S + 2:].any() and not op[1].any()
    flags = ssl.unpack(mask, tiles)
    spans = [ssl.tile_span_stated(t, TO, 48000, W) for t in range(tiles)]
    first_open = int(np.flatnonzero(op[0])[0])
    over = [t for t, (a, e) in enumerate(spans) if e > a0 and a < a1]
    assert len(over) >= 2 and flags[0, over].all(), "the tiles that span the carrier"
    lead_tiles = [t for t, (a, e) in enumerate(spans) if (e - 1) // S == first_open - 1]
    assert lead_tiles and flags[0, lead_tiles].all(), "the tiles that end in the slot in front of the first open one"
    last_open = int(np.flatnonzero(op[0])[-1])                # (hang 1: one slot behind the last carried one)
    assert last_open <= a1 // S + 1
    outside = [t for t, (a, e) in enumerate(spans) if (e - 1) // S + 1 < first_open or a // S > last_open]
    assert len(outside) > tiles // 2 and not flags[0, outside].any(), "the tiles beyond lead and hang"
    assert flags[0].sum() < 0.35 * tiles and not flags[1].any()
    assert int(state[0]) == 0 and int(state[1]) == 0


# ---- 5: the whole chain ----------------------------------------------------------------------------------------------------------------------------------------
FIRST = 2400 * 128   # the first block: 150 ms of noise alone, tuned unsquelched; its plane sets the levels, as the example's --squelch does


@functools.lru_cache(maxsize=None)
def _late_transmission(lead=FIRST + 4800 * 128):
    """A stream transmission at +12.5 kHz in a 2.048 MSPS int16 source: `lead` samples of noise alone — the first block and 300 ms of the second —, the
    transmission (40 ms of preamble, the link setup frame, six frames) and 200 ms of noise alone."""
    bb = ol.generate(ol.gen_params(seed=1, kind=1, lead_in=1920, n_frames=6, tail=960))
    sig = wl.wideband([bb], [12500.0], 128, fmt=wl.IQ_F32, sigma=0.0)[::3].astype(np.complex128)
    tail = 3200 * 128
    n = (lead + sig.size + tail) // 128 * 128
    x = np.zeros(n, dtype=np.complex128)
    x[lead:lead + sig.size] = sig
    rng = np.random.default_rng(6202)
    x += tr.SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    row = np.clip(np.rint(np.stack([x.real, x.imag], axis=-1)), -32768, 32767).astype(np.int16)
    row.setflags(write=False)
    return bb, row


def test_a_transmission_that_begins_inside_a_block_is_decoded_whole_from_the_slot_squelched_feed():
    """The receiver's order of calls: the first block is tuned unsquelched and its plane gives the levels (10 and 6 dB over the median floor); the second
    block, in which the transmission begins after 300 ms of noise, is tile-squelched at lead 1 and hang 1.  The demodulator has the first block's noise in
    front of the zeros, and 13 005 of them (17 closed tiles): the float oracle's carrier detect reads a long run of exact zeros as a carrier and false-locks on the edge
    behind it, squelch or no squelch — from its very first sample 3840 zeros do, behind noise 19 000 do and 16 000 do not (a property of the demodulator,
    measured while this test was written: the block squelch of ABI 619 feeds it the same zeros)."""
    bb, row = _late_transmission()
    expect = tr._good(ol.demod(bb)[0])
    assert len(expect) == 7
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    TO = rl.tile_outputs(taps1.size, tr.CH_R1, taps2.size, tr.CH_U, tr.CH_D)
    ratio = tr.CH_R1 * tr.CH_D / tr.CH_U
    fcw = [m17hip.wide_fcw(12500.0, ratio), m17hip.wide_fcw(-600000.0, ratio)]
    B = m17hip.wide_squelch_half_bins(9000.0, RATE, POINTS)
    feed = ssl.Feed([rl.Resampler(taps1, tr.CH_R1, tr.CH_U, tr.CH_D, taps2, w) for w in fcw], [0, 0], [row], POINTS, HOP, TO)
    Y0, P0, U0, dec0 = feed.block(0, FIRST)
    assert dec0 is None and np.array_equal(_u32(Y0), _u32(U0))
    p0, J0, _ = spl.plane(row[:FIRST], POINTS, HOP)
    o, c = m17hip.wide_squelch_levels(p0[None, :], J0, B, OPEN_DB, CLOSE_DB)
    feed.squelch = ssl.SlotSquelch([0, 0], fcw, o, c, B, 1, 1)
    Y, P, U, dec = feed.block(FIRST, row.shape[0])                        # ONE block: the transmission begins 300 ms into it
    state, bd, op, mask, tiles, J = dec
    plain = tr._good(fl.demod(np.concatenate([U0[0], U[0]]))[0])
    assert [p for _, p in plain] == [p for _, p in expect] and plain[0][0] == expect[0][0], "the unsquelched feed must decode every record, LSF included"
    got = tr._good(fl.demod(np.concatenate([Y0[0], Y[0]]))[0])
    assert got == plain, (len(got), len(plain))
    flags = ssl.unpack(mask, tiles)
    print(f"{int(flags[0].sum())} of {tiles} tiles of {TO} outputs open")
    assert 0 < flags[0].sum() < tiles and not flags[1].any(), (int(flags[0].sum()), tiles)
    assert not flags[0, 0] and (_u32(Y[0, :TO]) == 0).all() and (_u32(Y[1]) == 0).all()
    t0 = int(np.flatnonzero(flags[0])[0])                                 # the first open tile: its first output is the unsquelched word, not +0
    assert _u32(Y[0, t0 * TO]) == _u32(U[0, t0 * TO]) != 0 and np.array_equal(_u32(Y[0, t0 * TO:(t0 + 1) * TO]), _u32(U[0, t0 * TO:(t0 + 1) * TO]))
