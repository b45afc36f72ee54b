"""GPU tests of the forms resample_kernel (csrc/m17_resample_kernels.hpp) takes inside one tile.  tests/test_gpu_resample_input.py places its blocks on the
tile's own edges (G - 1, G, G + 1 groups), which reaches stage 2 with one chain or with four; here a block's size is chosen so that a tile holds a GIVEN
number of groups: g U outputs are a lone tile of g groups, (G + g) U outputs a full tile with a tail of g groups behind it whose front z is recomputed.
  1  resample_chains<1 .. 4, false> and <4, true> at the counts where the last chain is one lane, where the clamp to `kmax` and the `k > groups` drop
     decide single outputs: 63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193, 254 and 255 groups, with several residue classes;
  2  the eight-tap batch loop and its tail: classes of 7, 8 and 9 taps;
  3  tiles whose own G lies in each of the four bands, with up > 1;
  4  fewer than 64 u per chain in stage 1 beside several classes, and a tile that takes every byte of the 64 KB.
Every comparison is exact: the floats (m17hip_download_f32) as uint32 words against the HOST form (resample_lib.resample), NaN-ness where that is a NaN.
Every block is a fresh feed (m17hip_demod_reset first), so each T is a prefix of one expectation computed once per case.  3 channels on sources 0, 1, 0 of
3 (source 2 is heard by nobody), rows of an odd pitch, both gains, the host and the device form by turns; the frequency words go round 0, INT32_MIN, 1 and
-1 beside random ones.  Each test first asserts the tile resample_lib.tile gives (test_resample_input.TILES: the figures are restated there and checked
without a GPU): under another rule the T chosen here would no longer be the edges, and the test fails."""
import numpy as np
import pytest

import m17hip
import resample_lib as rl
import test_gpu_resample_input as gr
import test_gpu_wide2_input as g2
import test_resample_input as cpu
import wide_lib as wl

pytestmark = pytest.mark.gpu

FMTS, GAINS, INT32_MIN = gr.FMTS, gr.GAINS, gr.INT32_MIN
_assert_words, _dev, _raw = gr._assert_words, gr._dev, gr._raw
HOP_S, HOP_SRC, BAD_SRC = g2.HOP_S, g2.HOP_SRC, g2.BAD_SRC
CN = 3
WORDS = (0, INT32_MIN, 1, -1)
WAVE = 64


def _tile_is(case):
    R1, U, D, L1, L2 = case
    G, Q, lds = rl.tile(L1, R1, L2, U, D)
    assert (G, Q, lds) == cpu.TILES[case], (case, G, Q, lds)
    return G, Q


def _groups(T, U, G):
    """The groups each tile of a block of T outputs holds."""
    n = T // U
    return [G] * (n // G) + ([n % G] if n % G else [])


def _form(g):
    """The instantiation of resample_chains a tile of g groups takes: (chains, whether every k of them is one of the tile)."""
    return min(g // WAVE + 1, 4), g == 255


def _run(case, fmt, ts, turn):
    """Blocks of ts outputs of one case, each a fresh feed, against the host form.  `turn` moves the frequency words, the gains and the ways in on by one
    from case to case.  Returns the groups of every tile that ran."""
    R1, U, D, L1, L2 = case
    f = FMTS[fmt]
    ts = sorted(set(ts))
    Tmax = max(ts)
    rng = np.random.default_rng(6170 + 7 * f + R1 * D + U + L2)
    W = rl.row_len(Tmax, R1, U, D)
    P = W + 3   # odd: no row but 0 (and, of floats, 2) begins 16-byte aligned
    host = g2._hop_data(f, P, rng)
    dev = _dev(host)
    fcw = rng.integers(INT32_MIN, 1 << 31, CN).astype(np.int64)
    fcw[0], fcw[2] = WORDS[turn % 4], WORDS[(turn + 1 + turn // 4 % 3) % 4]   # (two different ones; channel 1 keeps a random word)
    src = HOP_SRC[:CN]
    assert src.tolist() == [0, 1, 0] and HOP_S == 3
    taps1, taps2 = gr._taps(rng, L1), gr._taps(rng, L2)
    exp = {g: np.stack([rl.resample(host[src[c]][:W], taps1, R1, U, D, taps2, int(fcw[c]), g) for c in range(CN)]) for g in GAINS}
    if f == wl.IQ_F32:   # (sample 3 of the bad source is infinite: the first outputs hold it whatever the taps)
        assert np.isnan(exp[1.0][BAD_SRC]).any() and np.isfinite(exp[1.0][0::2]).all()
    else:
        assert np.isfinite(exp[1.0]).all() and np.unique(gr._u32(exp[1.0])).size > exp[1.0].size // 2
    G = cpu.TILES[case][0]
    ran = []
    ctx = m17hip.Context(CN, Tmax)
    try:
        assert gr._resample(ctx, HOP_S, R1, taps1, U, D, taps2, f) == 0
        ctx.wide_channels(src, fcw)
        for ti, T in enumerate(ts):
            way = ("host", "device")[(ti + turn) & 1]
            gain = GAINS[((ti + turn) >> 1) & 1]
            ctx.reset()   # (a fresh feed: histories, count and carries are zero; every T is a prefix of the one expectation)
            name, ptr = ("m17hip_upload_wide", host.ctypes.data) if way == "host" else ("m17hip_upload_wide_device", dev.data_ptr())
            assert _raw(ctx, name, ptr, CN, T, P, gain) == 0, (case, fmt, T, way, "the launch is refused")
            ctx.C, ctx.T = CN, T
            _assert_words(ctx.download_f32(), exp[gain][:, :T], (case, fmt, _groups(T, U, G), T, gain, way))
            ran += _groups(T, U, G)
    finally:
        ctx.close()
    return ran


# ---- 1: chain counts at their edges ------------------------------------------------------------------------------------------------------------------
# (decim1, up, down, ntaps1, ntaps2), all G = 255 and Q = 64 with few taps: J2 = 4, JD = 2; J2 = 3, JD = 1 (the k = 0 sums read the padding in front of
# plane 0); J2 = 6, JD = 2 (the sub-filters' history fills the JD D u in front of the tile exactly); J2 = 8 (every class has exactly 8 taps: one batch of
# the tap loop and no tail)
CHAIN_CASES = [(2, 2, 3, 5, 7), (3, 5, 6, 7, 11), (2, 2, 3, 5, 12), (2, 3, 4, 9, 24)]
CHAIN_LONE = (63, 64, 65, 127, 128, 129, 191, 192, 193, 254)   # groups of a lone tile
CHAIN_TAIL = (64, 128, 192)                                     # groups of a tail behind a full tile
CHAIN_PARAMS = [(c, "i16") for c in CHAIN_CASES] + [(CHAIN_CASES[0], "f32"), (CHAIN_CASES[0], "u8")]


@pytest.mark.parametrize("case,fmt", CHAIN_PARAMS, ids=["{}_{}over{}_{}_{}-{}".format(*c, f) for c, f in CHAIN_PARAMS])
def test_every_chain_count_at_its_edges(case, fmt):
    """A tile of 63 groups is one chain; of 64, two, the second a single lane (k = 64) and every other lane of it clamped and dropped; 65 adds one lane; and
    so on through 128 and 192 to 254, and 255 — the full tile in front of a tail — is the form with no clamp at all.  The float source holds infinities and
    NaNs, which stay in the channel that listens to it."""
    G, Q = _tile_is(case)
    assert (G, Q) == (255, 64)
    U = case[1]
    ran = _run(case, fmt, [g * U for g in CHAIN_LONE] + [(G + g) * U for g in CHAIN_TAIL], CHAIN_PARAMS.index((case, fmt)))
    assert {_form(g) for g in ran} == {(1, False), (2, False), (3, False), (4, False), (4, True)}
    assert set(ran) == set(CHAIN_LONE) | {255}


# ---- 2: the batch loop's tail --------------------------------------------------------------------------------------------------------------------------
TAIL_CASES = [(1, 3, 4, 1, 25), (1, 3, 4, 1, 23)]   # classes of 9, 8 and 8 taps; of 8, 8 and 7


def _class_taps(U, D, L2):
    return [len(range(((r + 1) * D - 1) % U, L2, U)) for r in range(U)]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "{}_{}over{}_{}_{}".format(*c))
def test_classes_of_7_8_and_9_taps(case):
    """The taps of a class go eight at a time, the rest one by one: 9 is a batch and one, 8 a batch alone, 7 no batch at all."""
    G, Q = _tile_is(case)
    R1, U, D, L1, L2 = case
    assert sorted(_class_taps(U, D, L2)) == ([8, 8, 9] if L2 == 25 else [7, 8, 8])
    ran = _run(case, "i16", [U, 64 * U, 65 * U, 255 * U, 256 * U], 6 + TAIL_CASES.index(case))
    assert ran == [1, 64, 65, 255, 255, 1]


# ---- 3: tiles whose own G lies in each band, up > 1 ------------------------------------------------------------------------------------------------------
BAND_CASES = [(1, 32, 33, 1, 265), (1, 12, 31, 1, 249), (1, 12, 23, 1, 185), (1, 32, 91, 1, 729)]   # G = 121, 183, 226, 63: two, three, four chains, one
BAND_PARAMS = [(c, "i16") for c in BAND_CASES] + [(BAND_CASES[0], "u8")]


@pytest.mark.parametrize("case,fmt", BAND_PARAMS, ids=["{}_{}over{}_{}_{}-{}".format(*c, f) for c, f in BAND_PARAMS])
def test_tiles_whose_own_size_lies_in_each_band(case, fmt):
    """The rule's G is below 255 where the LDS is the limit: the full tile itself is then a clamped form (never <4, true>), with 12 or 32 classes."""
    G, Q = _tile_is(case)
    U = case[1]
    assert Q == 64 and _form(G) == {121: (2, False), 183: (3, False), 226: (4, False), 63: (1, False)}[G]
    ran = _run(case, fmt, [(G - 1) * U, G * U, (G + 1) * U, (2 * G + 1) * U], 8 + BAND_PARAMS.index((case, fmt)))
    assert ran == [G - 1, G, G, 1, G, G, 1]


# ---- 4: Q < 64 beside several classes, and all of the LDS ------------------------------------------------------------------------------------------------
FULL_CASES = [(16, 2, 115, 256, 4096), (16, 2, 15, 129, 4096), (16, 2, 7, 256, 4096)]   # Q = 57, 63, 58; the last one: 65 536 bytes
FULL_PARAMS = [(c, "i16") for c in FULL_CASES] + [(FULL_CASES[0], "f32")]


@pytest.mark.parametrize("case,fmt", FULL_PARAMS, ids=["{}_{}over{}_{}_{}-{}".format(*c, f) for c, f in FULL_PARAMS])
def test_partial_waves_in_stage_1_beside_two_classes_and_all_of_the_lds(case, fmt):
    """Stage 1 with fewer than 64 u per chain (wide_chains<0>, lanes Q .. 63 idle) feeding two classes of 2048 taps; (16, 2, 7, 256, 4096) asks for exactly
    the 64 KB a workgroup may have (resample_q accepts fixed + chunk == room): it must launch, and its words are the host form's."""
    G, Q = _tile_is(case)
    U = case[1]
    assert Q < 64 and (case != FULL_CASES[2] or cpu.TILES[case][2] == rl.LDS_LIMIT)
    ts = [U, G * U, (G + 1) * U] + ([(2 * G + 1) * U] if case == FULL_CASES[0] else [])
    ran = _run(case, fmt, ts, 13 + FULL_PARAMS.index((case, fmt)))
    assert ran[:4] == [1, G, G, 1]
