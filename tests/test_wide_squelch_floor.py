"""CPU-only: the sources' noise floor on the device (ABI 621, include/m17hip.h: m17hip_wide_squelch_floor, m17hip_wide_squelch_floor_fetch).  1: what the new
calls promise without a GPU.  2: the HOST form (detail/core.h's squelch_floor_key, squelch_floor_median, squelch_floor, squelch_track under the host
compiler, tests/cxx/squelch_floor_oracle.cpp) against a statement in Python integers and numpy on crafted rows, bit for bit.  3: against the existing path —
the levels are the words of "median of the fetched plane", and both squelch host forms fed them decide as they decide on the same levels given.  4: what it
is for — a source whose floor rises by 12 dB opens every channel under levels given once, and none under the floor taken per block."""
import ctypes as C
import functools

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol
import resample_lib as rl
import spectrum_lib as spl
import squelch_floor_lib as sf
import squelch_lib as sq
import squelch_slots_lib as ssl
import test_resample_input as tr

OPEN = sq.OPEN
NAN = sf.NAN
_u32, _f32 = sf.u32, sf.f32


def _word(v):
    return int(np.asarray(v, dtype=np.float32).reshape(-1).view(np.uint32)[0])


# ---- 1: exports, refusals and the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_squelch_floor", "m17hip_wide_squelch_floor_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 621
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert callable(m17hip.Context.wide_squelch_floor) and callable(m17hip.Context.wide_squelch_floor_fetch)
    assert m17hip.KERNELS["squelch_floor"] == 19 and m17hip.KERNELS["squelch_slots"] == 18
    assert len(set(m17hip.KERNELS.values())) == len(m17hip.KERNELS)
    r = m17hip.wide_squelch_ratio(10.0)
    assert isinstance(r, np.float32) and r == np.float32(10.0) and m17hip.wide_squelch_ratio(0.0) == np.float32(1.0)
    assert _u32(m17hip.wide_squelch_ratio(6.0)) == _u32(np.float32(10.0 ** 0.6))


def test_a_null_context_and_arguments_out_of_range_are_refused_and_nothing_is_written():
    lib = m17hip.load_library()
    inf, nan = float("inf"), float("nan")
    cases = [(10.0, 4.0, 1.0, 1.0, 0.0), (0.0, 0.0, 1.0, 1.0, 0.0),                                           # (in range: the NULL context alone)
             (nan, 4.0, 1.0, 1.0, 0.0), (10.0, inf, 1.0, 1.0, 0.0), (10.0, 4.0, nan, 1.0, 0.0), (10.0, 4.0, 1.0, -inf, 0.0), (10.0, 4.0, 1.0, 1.0, inf),
             (4.0, 10.0, 1.0, 1.0, 0.0), (10.0, 0.0, 1.0, 1.0, 0.0), (10.0, -1.0, 1.0, 1.0, 0.0), (0.0, -0.5, 1.0, 1.0, 0.0),
             (10.0, 4.0, 0.0, 1.0, 0.0), (10.0, 4.0, 1.5, 1.0, 0.0), (10.0, 4.0, 1.0, 0.0, 0.0), (10.0, 4.0, 1.0, 1.0000001, 0.0), (10.0, 4.0, 1.0, 1.0, -1.0e-30)]
    for o, c, r, f, m in cases:
        assert lib.m17hip_wide_squelch_floor(C.c_void_p(), C.c_float(o), C.c_float(c), C.c_float(r), C.c_float(f), C.c_float(m)) == -1, (o, c, r, f, m)
    plane = np.full(16, 7.0, dtype=np.float32)
    n, frames = C.c_uint32(78), C.c_uint32(79)
    for back in (0, 1, 2):
        assert lib.m17hip_wide_squelch_floor_fetch(C.c_void_p(), C.c_uint32(back), ol._p(plane), C.c_uint64(16), C.byref(n), C.byref(frames)) == -1
        assert lib.m17hip_wide_squelch_floor_fetch(C.c_void_p(), C.c_uint32(back), None, C.c_uint64(16), None, None) == -1
    assert (plane == 7.0).all() and (n.value, frames.value) == (78, 79)


# ---- 2: the host form against a statement of its own ---------------------------------------------------------------------------------------------------------
def test_the_key_orders_powers_as_unsigned_words_and_every_nan_last():
    vals = [0.0, 1.0e-45, 1.1754942e-38, 1.17549435e-38, 1.0, 3.0e38, float("inf")]
    keys = [sf.key(v) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys[0] == 0 and keys[-1] == 0x7F800000
    for word in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF):
        row = np.array([word], dtype=np.uint32).view(np.float32)
        assert int(sf.keys_stated(row)[0]) == 0xFFFFFFFF and sf.median(row) == NAN


def _rows(N):
    """name -> (row float32 [N], the expected median word, or None where the statement alone says it)."""
    rng = np.random.default_rng(6210 + N)
    h = N // 2
    out = {}
    out["all equal"] = (np.full(N, 3.5, dtype=np.float32), _word(np.float32(3.5)))
    ties = np.array([1.0] * (h - 3) + [2.0] * 6 + [3.0] * (N - h - 3), dtype=np.float32)
    out["ties across the rank"] = (rng.permutation(ties), _word(np.float32(2.0)))
    for raised, word in ((h - 1, 1.0), (h, 100.0), (h + 1, 100.0)):   # (where the upper median stops being the floor: at half the bins)
        r = np.full(N, 1.0, dtype=np.float32)
        r[rng.permutation(N)[:raised]] = 100.0
        out[f"{raised} bins raised"] = (r, _word(np.float32(word)))
    base = (rng.standard_normal(N) ** 2 * 10.0 ** rng.uniform(-3, 9, N)).astype(np.float32)
    for name, word in (("a +NaN", 0x7FC00000), ("a -NaN", 0xFFC00000)):
        r = base.copy()
        r.view(np.uint32)[5] = word
        finite = np.sort(np.delete(base, 5))
        out[name] = (r, _word(finite[h]))
    for nans, exp in ((h - 1, None), (h, NAN), (h + 1, NAN)):
        r = base.copy()
        r[rng.permutation(N)[:nans]] = np.nan
        out[f"{nans} NaNs"] = (r, _word(np.sort(r[~np.isnan(r)])[-1]) if exp is None else exp)
    r = base.copy()
    r[[0, 3, N - 1]] = np.inf
    out["three +inf"] = (r, None)
    r = base.copy()
    r[rng.permutation(N)[: h + 1]] = np.inf
    out["more than half +inf"] = (r, 0x7F800000)
    r = rng.integers(0, 0x800000, N).astype(np.uint32)   # (subnormals and +0: the word is the order)
    out["subnormal powers"] = (r.view(np.float32), int(np.sort(r)[h]))
    return out


@pytest.mark.parametrize("N", (64, 4096))
def test_the_median_is_the_key_of_rank_half_n(N):
    for name, (row, exp) in _rows(N).items():
        got, stated = sf.median(row), sf.median_stated(row)
        assert got == stated, (N, name, hex(got), hex(stated))
        assert exp is None or got == exp, (N, name, hex(got), hex(exp))
    # not np.median: on an even count that is the mean of the two middle values
    row = np.array([1.0] * (N // 2) + [3.0] * (N // 2), dtype=np.float32)
    assert sf.median(row) == _word(np.float32(3.0)) and np.median(row) == 2.0


def test_the_floor_is_two_rounded_operations_and_a_lower_bound():
    for med, B, J, fmin in ((1.1, 4, 100, 0.0), (3.3333333e7, 64, 1171, 0.0), (1.0e-38, 0, 7, 0.0), (7.0, 2, 3, 1.0e-3), (0.0, 4, 16, 0.0)):
        got = sf.floor(med, B, J, fmin)
        assert _u32(got) == _u32(sf.floor_stated(med, B, J, fmin)), (med, B, J)
    # two roundings, not one: the product is rounded before the division
    med, B, J = np.float32(1.0000001), 1, 3
    assert _u32(sf.floor(med, B, J, 0.0)) == _u32(np.float32(np.float32(med * np.float32(3.0)) / np.float32(3.0)))
    # floor_min above, below, and a NaN in
    assert sf.floor(2.0, 0, 1, 5.0) == np.float32(5.0) and sf.floor(2.0, 0, 1, 1.0) == np.float32(2.0) and sf.floor(0.0, 4, 9, 0.25) == np.float32(0.25)
    assert np.isnan(sf.floor(np.nan, 0, 1, 5.0)) and np.isnan(sf.floor(np.nan, 3, 10, 0.0))
    assert sf.floor(np.inf, 1, 2, 5.0) == np.float32(np.inf)


def test_the_track_on_crafted_pairs():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # from the NaN carry: the first block sets the floor, whatever it is
    assert sf.track(nan, 3.0, 0.125, 0.5) == np.float32(3.0) and sf.track(nan, inf, 0.125, 0.5) == inf and np.isnan(sf.track(nan, nan, 0.125, 0.5))
    # rising by an eighth, falling at once
    assert sf.track(8.0, 16.0, 0.125, 1.0) == np.float32(9.0) and sf.track(8.0, 2.0, 0.125, 1.0) == np.float32(2.0)
    assert sf.track(8.0, 8.0, 0.125, 0.25) == np.float32(8.0)
    # a non-finite floor holds the carry
    assert sf.track(8.0, inf, 0.125, 1.0) == np.float32(8.0) and sf.track(8.0, nan, 1.0, 1.0) == np.float32(8.0)
    # a factor of 1 returns f to the bit, where fmaf(1, f - F, F) does not: 2^-30 - 1 rounds to -1, and -1 + 1 is 0
    F, f = np.float32(1.0), np.float32(2.0 ** -30)
    d = np.float32(f - F)
    assert d == np.float32(-1.0) and sf.fma32(np.float32(1.0), d, F) == np.float32(0.0) != f
    assert _u32(sf.track(F, f, 0.125, 1.0)) == _u32(f) and _u32(sf.track(f, F, 1.0, 0.125)) == _u32(F)
    # the stated form, random pairs and factors
    rng = np.random.default_rng(6211)
    for _ in range(300):
        F, f = (rng.standard_normal(2) ** 2 * 10.0 ** rng.uniform(-6, 9, 2)).astype(np.float32)
        a, b = np.float32(rng.uniform(0.01, 1.0)), np.float32(rng.choice([1.0, 0.5, 0.3, 0.125]))
        assert _u32(sf.track(F, f, a, b)) == _u32(sf.track_stated(F, f, a, b)), (F, f, a, b)


def test_a_block_of_floors_is_the_stated_form_of_its_sources():
    rng = np.random.default_rng(6212)
    plane = (rng.standard_normal((3, 64)) ** 2 * 100.0).astype(np.float32)
    plane[1] = 0.0
    plane[2, :40] = np.nan
    fl_ = sf.Floor(3, 2, m17hip.wide_squelch_ratio(10.0), m17hip.wide_squelch_ratio(6.0), 0.125, 1.0, 0.0)
    for J, scale in ((3, 1.0), (0, 5.0), (5, 4.0), (2, 0.25)):
        carry = fl_.carry.copy()
        p = (plane * np.float32(scale)).astype(np.float32)
        got = fl_.block(p, J)
        exp = fl_.block_stated(p, J, carry)
        assert np.array_equal(_u32(got), _u32(exp)), (J, got, exp)
        assert np.array_equal(_u32(fl_.carry), _u32(got[1]))
        if J == 0:
            assert np.array_equal(_u32(fl_.carry), _u32(carry))
    assert fl_.carry[1] == 0.0 and _word(fl_.carry[2]) == NAN   # (a row of zeros: floor +0; a row of NaNs from the first block on: the carry stays a NaN)
    # levels of a NaN floor open every channel: the fail-open rule
    s = sq.Squelch([2, 2], [0, 1 << 30], got[2], got[3], 2, 0)
    state, _ = s.block(np.nan_to_num(plane), 3)
    assert ((state & OPEN) != 0).all()


# ---- 3 and 4: the 2.048 MSPS source of three transmissions ---------------------------------------------------------------------------------------------------
POINTS, HOP = 2048, 2048
OPEN_DB, CLOSE_DB, HANG = 10.0, 6.0, 1
EMPTY = (400000.0, -300000.0, 900000.0, 62500.0)   # Hz: nobody transmits there (tests/test_wide_squelch.py)
BLOCK = 4800                                        # outputs per block: 100 ms, 204 800 source samples, 100 frames
STEP = BLOCK // tr.CH_U * tr.CH_R1 * tr.CH_D
LOUD_FROM = 2                                       # the block from which the float source is 12 dB louder
RATE = 2048000.0


@functools.lru_cache(maxsize=None)
def _source():
    bb = [ol.generate(ol.gen_params(seed=1, kind=k, lead_in=9600, n_frames=6, tail=4800)) for k in tr.KINDS]
    x = tr.source_2048k(bb)
    x.setflags(write=False)
    return bb, x


@functools.lru_cache(maxsize=None)
def _loud_source():
    """The same in float32, the whole source times 4 from block LOUD_FROM on (exact: nothing clips)."""
    x = _source()[1].astype(np.float32)
    z = (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)
    z[LOUD_FROM * STEP:] *= np.float32(4.0)
    z.setflags(write=False)
    return z


def _cuts(n):
    return [(a, min(a + STEP, n)) for a in range(0, n, STEP)]


@functools.lru_cache(maxsize=None)
def _planes(loud):
    x = _loud_source() if loud else _source()[1]
    out, count = [], 0
    for a, b in _cuts(x.shape[0]):
        p, J, _ = spl.plane(x[a:b], POINTS, HOP, None, count)
        out.append((p[None, :], J))
        count += b - a
    return out


def _channels():
    offs = list(tr.OFFSETS) + list(EMPTY)
    return [m17hip.wide_fcw(f, tr.CH_R1 * tr.CH_D / tr.CH_U) for f in offs], m17hip.wide_squelch_half_bins(9000.0, RATE, POINTS)


def test_the_levels_are_the_median_of_the_fetched_plane_and_both_modes_take_them_as_given_levels():
    fcw, B = _channels()
    ro, rc = m17hip.wide_squelch_ratio(OPEN_DB), m17hip.wide_squelch_ratio(CLOSE_DB)
    floor = sf.Floor(1, B, ro, rc)
    x = _source()[1]
    a_floor, a_given = sq.Squelch([0] * 7, fcw, [1.0], [1.0], B, HANG), None
    s_floor, s_given = ssl.SlotSquelch([0] * 7, fcw, [1.0], [1.0], B, HANG, 1), None
    count = 0
    for (a, b), (plane, J) in zip(_cuts(x.shape[0]), _planes(False)):
        out = floor.block(plane, J)
        if J:
            # independently: np.partition on the keys, then the three rounded operations
            k = np.partition(sf.keys_stated(plane[0]), POINTS // 2)[POINTS // 2]
            med = _f32(k)
            f = np.float32(np.float32(med * np.float32(2 * B + 1)) / np.float32(J))
            assert np.array_equal(_u32(out[:, 0]), _u32([med, f, np.float32(f * ro), np.float32(f * rc)])), (a, out)
            # and it is what the Python layer's float64 median gives to within the two middle values' distance
            o64, _ = m17hip.wide_squelch_levels(plane, J, B, OPEN_DB, CLOSE_DB)
            assert abs(float(out[2, 0]) / float(o64[0]) - 1.0) < 0.05
        # the block mode: fed the levels per block, against a form that got them as given levels from the start (the hold counts carried over by hand)
        a_floor.open, a_floor.close = out[2].copy(), out[3].copy()
        a_given = sq.Squelch([0] * 7, fcw, out[2], out[3], B, HANG)
        a_given.hold[:] = a_floor.hold
        got, exp = a_floor.block(plane, J), a_given.block(plane, J)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(_u32(got[1]), _u32(exp[1]))
        # the slot mode likewise
        rows, Js, first = ssl.slot_rows(x[a:b], POINTS, HOP, None, count)
        assert Js == J
        s_floor.open, s_floor.close = out[2].copy(), out[3].copy()
        s_given = ssl.SlotSquelch([0] * 7, fcw, out[2], out[3], B, HANG, 1)
        s_given.hold[:] = s_floor.hold
        T = (b - a) // (tr.CH_R1 * tr.CH_D) * tr.CH_U
        got, exp = s_floor.block(rows[None], J, first, HOP, 255, T, b - a), s_given.block(rows[None], J, first, HOP, 255, T, b - a)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(_u32(got[1]), _u32(exp[1])) and np.array_equal(got[3], exp[3])
        count += b - a


def test_a_floor_that_rises_opens_everything_under_given_levels_and_nothing_under_the_floor_of_the_block():
    """The source in float32, 100 ms blocks, times 4 (12 dB) from block LOUD_FROM on; a band of 9 kHz, 10 / 6 dB, hang 1.  Levels given once from block 0: the
    four channels on empty spectrum are open in every louder block — the squelch saves nothing.  Levels from each block's own floor (rise = fall = 1):
    closed in every block that holds a frame, the three transmissions open throughout, and each decodes 7 of 7 records."""
    bb, _ = _source()
    x = _loud_source()
    fcw, B = _channels()
    planes = _planes(True)
    have = np.array([J > 0 for _, J in planes])
    assert have[: LOUD_FROM + 2].all()
    # given levels, taken from block 0 as the example program does
    o, c = m17hip.wide_squelch_levels(planes[0][0], planes[0][1], B, OPEN_DB, CLOSE_DB)
    given = sq.Squelch([0] * 7, fcw, o, c, B, HANG)
    opens = np.array([(given.block(p, J)[0] & OPEN) != 0 for p, J in planes])
    assert not opens[1:LOUD_FROM, 3:].any()                    # (the premise: while the floor stands, they are closed)
    assert opens[LOUD_FROM:, 3:].all(), opens[:, 3:]           # (the failure: every empty channel open in every louder block)
    # the floor of the block, through the whole chain for the three transmissions
    taps1, taps2 = m17hip.wide_resample_default_taps(tr.CH_R1, tr.CH_U, tr.CH_D)
    dec = sq.Squelch([0] * 7, fcw, [1.0], [1.0], B, HANG)
    dfl = sf.Floor(1, B, m17hip.wide_squelch_ratio(OPEN_DB), m17hip.wide_squelch_ratio(CLOSE_DB))
    opens = []
    for p, J in planes:
        out = dfl.block(p, J)
        dec.open, dec.close = out[2].copy(), out[3].copy()
        opens.append((dec.block(p, J)[0] & OPEN) != 0)
    opens = np.array(opens)
    assert opens[:, :3].all(), opens[:, :3]
    assert not opens[have][:, 3:].any(), opens[:, 3:]
    feed = sf.Feed([rl.Resampler(taps1, tr.CH_R1, tr.CH_U, tr.CH_D, taps2, w) for w in fcw[:3]], [0] * 3, [x], POINTS, HOP)
    feed.squelch = sq.Squelch([0] * 3, fcw[:3], [1.0], [1.0], B, HANG)
    feed.floor = sf.Floor(1, B, m17hip.wide_squelch_ratio(OPEN_DB), m17hip.wide_squelch_ratio(CLOSE_DB))
    ys = []
    for a, b in _cuts(x.shape[0]):
        Y, P, state, band, J, out = feed.block(a, b)
        assert ((state & OPEN) != 0).all()
        ys.append(Y)
    y = np.concatenate(ys, axis=1)
    for ch in range(3):
        got = fl.demod(y[ch])[0]
        assert len(tr._good(got)) == 7, tr.OFFSETS[ch]
