"""CPU-only: the raster survey (ABI 613, include/m17hip.h: m17hip_wide_survey — per-bin power of every source beside the channeliser).  1: the survey-time
rule is a property of the feed, not of its blocks.  2: the two-level sum at its group edges, word for word against a statement in Python, and it is NOT the
single chain.  3: the HOST form (tests/survey_lib.py: raster_lib's z, detail/core.h's chan_power and sum under the host compiler) against float64 within a
derived bound that a survey one output early misses.  4: the feature means something — the three transmissions of tests/test_raster_input.py stand out of
a 2.4 MSPS source's 192 bins.  5: exports, bindings, refusals that need no device, and wide_raster_occupied."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import iq_lib as iq
import m17hip
import oracle_lib as ol
import raster_lib as rl
import survey_lib as sl
import test_raster_input as tri
import wide_lib as wl

EINVAL = -1


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _noise(M, R, L, T, seed):
    rng = np.random.default_rng(seed)
    taps = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    x = rng.integers(-20000, 20001, size=(T * R, 2)).astype(np.int16)
    x.setflags(write=False)
    return x, taps


# ---- 1: the survey-time rule ----------------------------------------------------------------------------------------------------------------------------
RULE_LENS = (1, 2, 15, 1, 16, 17, 3, 33, 1, 1, 48, 7)   # outputs per block


@pytest.mark.parametrize("stride", [1, 2, 3, 16, 17])
def test_the_survey_times_of_a_cut_feed_are_the_uncut_feeds(stride):
    """(N0 + n + 1) % stride == 0: the union of the blocks' survey times, as feed outputs, is the uncut feed's, and J per block is the number of multiples of
    the stride in (N0, N0 + T] — blocks with J = 0 included.  The host form's feed (survey_lib.Survey) reports the same J and N0 block by block, and its
    planes are those of the z it is handed."""
    cuts = np.cumsum((0,) + RULE_LENS).tolist()
    T = cuts[-1]
    whole = sl.times(0, T, stride)
    assert whole.tolist() == [n for n in range(T) if (n + 1) % stride == 0]
    M, R, L = 6, 4, 13
    x, taps = _noise(M, R, L, T, 6130 + stride)
    feed = sl.Survey(taps, R, M, stride)
    _, zw = rl.Raster(taps, R, M, sl.all_bins(M)).block(x, want_z=True)
    got, js = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        t = sl.times(a, b - a, stride)
        J = b // stride - a // stride
        assert t.size == J
        plane, Jf, N0 = feed.block(x[a * R: b * R])
        assert (Jf, N0) == (J, a)
        assert np.array_equal(_u32(plane), _u32(sl.plane_of(zw[:, a:b], t)))
        if J == 0:
            assert (_u32(plane) == 0).all()   # (+0)
        got += [a + int(n) for n in t]
        js.append(J)
    assert got == whole.tolist()
    if stride > 1:
        assert 0 in js


# ---- 2: group edges -------------------------------------------------------------------------------------------------------------------------------------
def _round_f32(v):
    """The float32 nearest to the exact rational v, ties to even."""
    f = np.float32(float(v))
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - v)
        if best is None or d < best[0] or (d == best[0] and int(_u32(c)) & 1 == 0 and int(_u32(best[1])) & 1 == 1):
            best = (d, c)
    return best[1]


def _power_stated(re, im):
    """fmaf(re, re, im * im) in words of its own: the product im * im rounded to float32, the rest exact, rounded once."""
    prod = np.float32(im) * np.float32(im)
    return _round_f32(Fraction(float(re)) * Fraction(float(re)) + Fraction(float(prod)))


def _plane_stated(zrow, single=False):
    p = [_power_stated(z.real, z.imag) for z in zrow]
    if single:
        acc = np.float32(0.0)
        for v in p:
            acc = np.float32(acc + v)
        return acc
    P = np.float32(0.0)
    for g in range(0, len(p), 16):
        q = np.float32(0.0)
        for v in p[g: g + 16]:
            q = np.float32(q + v)
        P = np.float32(P + q)
    return P


def test_the_two_level_sum_at_its_group_edges_and_it_is_not_the_single_chain():
    """J = 15, 16, 17, 33 at stride 1: the host form's words are those of the definition stated in Python (an exactly rounded fma, float32 adds).  Up to 16
    times the two levels ARE the single chain; beyond they are not — on this data some bin differs in words, so the grouping is pinned."""
    M, R, L = 12, 4, 5
    x, taps = _noise(M, R, L, 33, 6140)
    _, z = rl.Raster(taps, R, M, sl.all_bins(M)).block(x, want_z=True)
    differs = {}
    for J in (15, 16, 17, 33):
        t = sl.times(0, J, 1)
        assert t.size == J
        two, one = sl.plane_of(z[:, :J], t), sl.plane_of(z[:, :J], t, single=True)
        assert np.array_equal(_u32(two), _u32([_plane_stated(z[k, :J]) for k in range(M)])), J
        assert np.array_equal(_u32(one), _u32([_plane_stated(z[k, :J], single=True) for k in range(M)])), J
        differs[J] = int((_u32(two) != _u32(one)).sum())
    print(f"bins of {M} whose two-level sum differs from the single chain: {differs}")
    assert differs[15] == 0 and differs[16] == 0
    assert differs[17] + differs[33] > 0, "the test data does not tell the two-level sum from a single chain"


# ---- 3: the host form against float64 -------------------------------------------------------------------------------------------------------------------
# survey_lib.plane_f64's docstring derives the bound from raster_lib.f64_bound: the error of |z|^2 from the bound on z, the rounding of chan_power and the
# adds a power passes through.  (M, decim, taps, outputs, stride)
F64_SHAPES = [s + (200, 3) for s in rl.SMALL] + [(192, 50, 1601, 120, 7)]


@pytest.mark.parametrize("shape", F64_SHAPES, ids=["M{}_R{}_L{}".format(*s[:3]) for s in F64_SHAPES])
def test_the_host_form_is_within_the_derived_bound_of_float64_and_a_survey_one_output_early_is_not(shape):
    """Largest measured |P_host - P64| over its bound: 0.0122 (M 12, decim 4, 5 taps); 0.0005 at M 192, decim 50, 1601 taps.  Surveyed one output early
    (output n in place of n + 1) the float64 statement is thousands of bounds away on the same data (2987 at the least)."""
    M, R, L, T, stride = shape
    x, taps = _noise(M, R, L, T, 6150 + M + R + L)
    worst = 0.0
    for count in (0, 5 * R):
        plane, J, N0 = sl.Survey(taps, R, M, stride, count=count).block(x)
        P64, B, J64 = sl.plane_f64(x, taps, R, M, stride, count=count)
        assert J == J64 and J >= T // stride and N0 == count // R
        ratio = np.abs(plane.astype(np.float64) - P64) / B
        worst = max(worst, float(ratio.max()))
        Pw, Bw, _ = sl.plane_f64(x, taps, R, M, stride, count=count, phase=0)
        early = float((np.abs(plane.astype(np.float64) - Pw) / Bw).max())
        print(f"survey vs float64, M {M} decim {R} taps {L} count {count}: {float(ratio.max()):.4f} of its bound; one output early {early:.1f}")
        assert float(ratio.max()) <= 1.0, (shape, count)
        assert early > 1.0, (shape, count)
    print(f"survey vs float64, M {M} decim {R} taps {L}: largest ratio {worst:.4f}")


# ---- 4: end to end at 2.4 MSPS on the host form alone ---------------------------------------------------------------------------------------------------
E2E_STRIDE = 48
MIN_GAP_DB = 6.0


@pytest.fixture(scope="module")
def basebands():
    out = []
    for kind in tri.KINDS:
        s = ol.generate(ol.gen_params(seed=1, kind=kind, lead_in=9600, n_frames=6, tail=4800))
        s.setflags(write=False)
        out.append(s)
    return out


def test_three_transmissions_stand_out_of_192_bins(basebands):
    """tests/test_raster_input.py's three transmissions at bins -61, 1 and 2 of a 2.4 MSPS int16 source with noise, surveyed at stride 48 over the whole
    burst.  Measured on the host form, in dB over the row's median: the weakest of the three occupied bins 36.94, the strongest of the other 189 9.88 (that is bin 0;
    bin 3 has 9.65: the two neighbours that take the adjacent-channel leakage ARE the strongest of the rest).  The test requires a gap of at least 6 dB between the two and puts the margin half way;
    wide_raster_occupied then reports exactly the three bins of source 0."""
    R, M = tri.E2E_R, tri.E2E_M
    bins = [m17hip.wide_bin(f, R, M) for f in tri.OFFSETS]
    assert bins == [-61, 1, 2]
    x = wl.wideband(basebands, tri.OFFSETS, R, amplitude=6000.0, sigma=tri.SIGMA, seed=1, fmt=wl.IQ_I16)
    plane, J, N0 = sl.Survey(m17hip.wide_raster_default_taps(R), R, M, E2E_STRIDE).block(x)
    assert N0 == 0 and J == (x.shape[0] // R) // E2E_STRIDE and J > 100
    db = 10.0 * np.log10(plane.astype(np.float64) / float(np.median(plane.astype(np.float64))))
    occ = [b % M for b in bins]
    rest = [k for k in range(M) if k not in occ]
    assert len(rest) == 189 and 0 in rest and 3 in rest
    weakest, strongest = float(db[occ].min()), float(db[rest].max())
    print(f"dB over the floor: weakest occupied bin {weakest:.2f}, strongest other bin {strongest:.2f} (bin 0 {db[0]:.2f}, bin 3 {db[3]:.2f})")
    assert weakest - strongest >= MIN_GAP_DB, (weakest, strongest)
    margin = 0.5 * (weakest + strongest)
    found = m17hip.wide_raster_occupied(plane[None, :], margin)
    assert sorted((s, b) for s, b, _ in found) == [(0, -61), (0, 1), (0, 2)]
    assert [d for _, _, d in found] == sorted((d for _, _, d in found), reverse=True)
    assert all(abs(d - db[b % M]) < 1e-9 for _, b, d in found)


# ---- 5: exports, refusals, the Python layer -------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_wide_survey", "m17hip_wide_survey_fetch"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 613
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for f in (m17hip.Context.wide_survey, m17hip.Context.wide_survey_fetch, m17hip.wide_raster_occupied):
        assert callable(f)
    assert m17hip.KERNELS["survey"] == 12 and m17hip.KERNELS["channelise"] == 11
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(iq.ROOT, "m17-cxx-demod_amd", "libm17hip.so")], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(iq.ROOT, "include", "m17hip.h")).read()
    for name in NEW:
        assert f" T {name}\n" in out and f"int {name}(" in header, name
    cxx = open(os.path.join(iq.ROOT, "m17-cxx-demod_amd", "include", "m17cxx", "BatchedDemodulator.h")).read()
    assert "void wide_survey(uint32_t stride)" in cxx and "void wide_survey_fetch(" in cxx
    core = open(iq.CORE).read()
    assert "CHAN_SURVEY_GROUP = 16" in core and "float chan_power(float re, float im)" in core


def test_refusals_that_need_no_device():
    lib = m17hip.load_library()
    buf = np.full(8, 7.0, dtype=np.float32)
    t, n0 = C.c_uint32(9), C.c_uint64(9)
    assert lib.m17hip_wide_survey(None, C.c_uint32(1)) == EINVAL
    assert lib.m17hip_wide_survey(None, C.c_uint32(4097)) == EINVAL
    for back in (0, 1, 2):
        assert lib.m17hip_wide_survey_fetch(None, C.c_uint32(back), ol._p(buf), C.c_uint64(buf.size), C.byref(t), C.byref(n0)) == EINVAL
    assert (buf == 7.0).all() and t.value == 9 and n0.value == 9
    with pytest.raises(m17hip.M17HipError):
        m17hip.Context.wide_survey_fetch(None, back=2)   # (refused before the context is looked at)


def test_wide_raster_occupied():
    M = 12
    p = np.ones((4, M), dtype=np.float32)
    p[0, 1], p[0, 7], p[0, 6] = 100.0, 1000.0, 10.0      # bins 1, -5 and -6 of source 0 at 20, 30 and 10 dB
    p[1] = 0.0
    p[1, 3] = 5.0                                       # a row whose median is 0
    p[2, :7] = np.nan                                   # a row whose median is not finite
    p[3, 5] = np.inf                                    # an infinite bin over a finite floor
    got = m17hip.wide_raster_occupied(p, 15.0)
    assert [(s, b) for s, b, _ in got] == [(3, 5), (0, -5), (0, 1)]
    assert got[0][2] == np.inf and abs(got[1][2] - 30.0) < 1e-9 and abs(got[2][2] - 20.0) < 1e-9
    assert [(s, b) for s, b, _ in m17hip.wide_raster_occupied(p[0], 5.0)] == [(0, -5), (0, 1), (0, -6)]
    assert m17hip.wide_raster_occupied(p[1:3], -100.0) == []
