"""GPU tests of the tuners' phase across a sample count of 2^32 (include/m17hip.h: the oscillator's phase is fcw * m mod 2^32, m the feed's sample index).  The
host form has been taken across that count on the CPU (tests/test_wide_input.py, tests/test_wide2_input.py); here the DEVICE's feed is: one uint8 source and
one channel at an odd frequency word, advanced with in-place device blocks of one reused random device buffer (their floats are not looked at) until 300
outputs are left before the count wraps, then blocks of 1, 255 and 300 outputs (the resampler, whose blocks are whole groups of `up` outputs: 3, 255 and
300) across the wrap whose words are the host form's — started at that count, with the history and the carry the last long block left.  2^32 samples are
30 minutes at 2.4 MSPS, 35 at 2.048 MSPS and 93 minutes at 768 kSPS: a receiver gets there."""
import numpy as np
import pytest

import m17hip
import resample_lib as rl
import test_gpu_wide_input as g1
import wide2_lib as w2
import wide_lib as wl

pytestmark = pytest.mark.gpu

_u32, _assert_words, _dev = g1._u32, g1._assert_words, g1._dev
BIG = 1 << 28                 # samples of the reused buffer: 512 MB of uint8 pairs
WRAP = 1 << 32
BEFORE = 300                  # outputs left before the wrap when the short blocks begin
CROSS = (1, 255, 300)         # outputs per short block: the third one crosses
FCW = -0x12345679             # odd: the phase takes every residue, no power of two divides the count out of it


@pytest.fixture(scope="module")
def big():
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(6120)
    t = torch.randint(0, 256, (BIG, 2), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()   # (complete before it is handed over: the context's streams do not wait for torch's)
    yield t
    del t
    torch.cuda.empty_cache()


def _across(ctx, big, make, R, H, per_block, what, per=1, cross=CROSS):
    """The feed of `ctx` (configured, one channel on source 0 at FCW) advanced until BEFORE outputs are left before WRAP samples, then `cross`; a group of R
    samples gives `per` outputs (1 for the integer tuners; down * decim1 samples per `up` outputs for the resampler, whose blocks are whole groups);
    `make(count)` is a host-form tuner of the same configuration with a zero history and carry."""
    assert BEFORE % per == 0 and all(n % per == 0 for n in cross)
    start = WRAP - BEFORE // per * R
    assert per_block % R == 0 and per_block <= BIG and start % R == 0
    count = 0
    while count < start:
        last = min(per_block, start - count)
        ctx.upload_wide_device(big.data_ptr(), 1, last // R * per, BIG)
        count += last
    # the host form at that count: the history is the last H converted samples of the last long block, the carry that block's last z — both from a
    # host-form run over the block's tail, begun (from zeroes, which the last output no longer sees) at the count the tail had
    N = -(-H // R) + 2
    assert N * R >= H + R and N * R <= last
    tail = big[last - N * R: last].cpu().numpy()
    t = make(start - N * R)
    t.block(tail)
    assert t.count == start
    zero = make(0)
    zero.hist[:] = t.hist
    zero.carry[:] = t.carry
    rng = np.random.default_rng(6121 + R)
    x = rng.integers(0, 256, size=(sum(cross) // per * R, 2)).astype(np.uint8)
    dev = _dev(x)
    a = 0
    for n in cross:
        lo, hi = a // per * R, (a + n) // per * R
        ctx.upload_wide_device(dev.data_ptr() + lo * 2, 1, n, x.shape[0])
        e, other = t.block(x[lo:hi]), zero.block(x[lo:hi])
        assert e.size == n
        assert not np.array_equal(_u32(e), _u32(other)), "the count matters: the same block from count 0 is other words"
        _assert_words(ctx.download_f32(), e[None, :], (what, "outputs", a, a + n))
        a += n
    assert t.count == WRAP + (sum(cross) - BEFORE) // per * R and sum(cross) > BEFORE and sum(cross[:-1]) < BEFORE


def test_two_stage_feed_across_2_to_the_32_samples(big):
    """16 x 16, 33 / 65 taps (58 u per chain of a chunk): sixteen blocks of 2^28 samples, the last one 300 outputs short."""
    R1, R2, L1, L2 = 16, 16, 33, 65
    R = R1 * R2
    taps1, taps2 = wl.hamming_taps(L1), wl.hamming_taps(L2)
    ctx = m17hip.Context(1, BIG // R)
    try:
        ctx.wide_config2(1, R1, R2, wl.IQ_U8, taps1, taps2)
        ctx.wide_channels([0], [FCW])
        ctx.reset()
        _across(ctx, big, lambda count: w2.Tuner2(taps1, R1, taps2, R2, FCW, 1.0, count=count), R, w2.hist_len(L1, R1, L2), BIG, "two stages")
    finally:
        ctx.close()


def test_single_stage_feed_across_2_to_the_32_samples(big):
    """R = 16, 33 taps: sixty-four blocks of 2^26 samples (4 194 304 outputs each), the last one 300 outputs short."""
    R, L = 16, 33
    taps = wl.hamming_taps(L)
    per_block = 1 << 26
    ctx = m17hip.Context(1, per_block // R)
    try:
        ctx.wide_config(1, R, wl.IQ_U8, taps)
        ctx.wide_channels([0], [FCW])
        ctx.reset()
        _across(ctx, big, lambda count: wl.Tuner(taps, R, FCW, 1.0, count=count), R, L - 1, per_block, "one stage")
    finally:
        ctx.close()


def test_resampling_feed_across_2_to_the_32_samples(big):
    """16 x 3 / 8 (2.048 MSPS: the count wraps after 35 minutes), 33 / 65 taps: sixteen blocks of 2^28 samples — 3 x 2^21 outputs each —, the last one 100
    groups short, then blocks of 3, 255 and 300 outputs.  resample_kernel adds count + k in its own text, on the path that loads whole groups of samples
    and on the one that goes sample by sample (the history, the block's edges)."""
    R1, U, D, L1, L2 = 16, 3, 8, 33, 65
    assert rl.tile(L1, R1, L2, U, D) == (255, 64, 55672)
    group = R1 * D
    taps1, taps2 = wl.hamming_taps(L1), wl.hamming_taps(L2)
    ctx = m17hip.Context(1, BIG // group * U)
    try:
        ctx.wide_resample(1, R1, U, D, wl.IQ_U8, taps1, taps2)
        ctx.wide_channels([0], [FCW])
        ctx.reset()
        _across(ctx, big, lambda count: rl.Resampler(taps1, R1, U, D, taps2, FCW, 1.0, count=count), group, rl.hist_len(L1, R1, L2, U), BIG, "resampler",
                per=U, cross=(3, 255, 300))
    finally:
        ctx.close()
