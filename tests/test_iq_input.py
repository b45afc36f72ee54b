"""CPU-only: complex IQ input (ABI 608, include/m17hip.h: m17hip_upload_iq and friends).  1: the arithmetic of the discriminator's HOST form
(detail/core.h under the host compiler, tests/cxx/iq_oracle.cpp) — fm_phase within 2^-20 rad of float64 atan2, odd in its second argument to the bit, +0
for a zero product; fm_cross product by product.  2: the feature means something — a frequency-modulated transmission, discriminated by the host form
and demodulated by the float oracle, carries the frames the int16 oracle finds in the baseband itself.  3: the feed rule on the host form.  4: what the
new calls promise without a GPU: the symbols, the version, a null context refused."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import f32_lib as fl
import iq_lib as iq
import m17hip
import oracle_lib as ol

BOUND = 2.0 ** -20
TINY, HUGE = np.float32(1e-30), np.float32(1e30)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """(re, im): 1.2e6 random pairs with magnitudes over 1e-3 .. 1e9, 2e5 within 1e-3 relative of the axes and the diagonals, and {0, +-1, +-tiny, +-huge}^2."""
    rng = np.random.default_rng(608)
    n = 1_200_000
    mag = 10.0 ** rng.uniform(-3, 9, n)
    th = rng.uniform(-np.pi, np.pi, n)
    re, im = [mag * np.cos(th)], [mag * np.sin(th)]
    m = 200_000
    mag = 10.0 ** rng.uniform(-3, 9, m)
    th = rng.integers(0, 8, m) * (np.pi / 4) + rng.uniform(-1e-3, 1e-3, m)
    re.append(mag * np.cos(th))
    im.append(mag * np.sin(th))
    special = [0.0, -0.0, 1.0, -1.0, TINY, -TINY, HUGE, -HUGE]
    sp = np.array(list(itertools.product(special, special)), dtype=np.float32)
    re.append(sp[:, 0])
    im.append(sp[:, 1])
    re = np.concatenate(re).astype(np.float32)
    im = np.concatenate(im).astype(np.float32)
    assert np.isfinite(re).all() and np.isfinite(im).all()
    return re, im


def test_phase_is_within_the_bound_of_float64_atan2(pairs):
    re, im = pairs
    got = iq.phase(re, im).astype(np.float64)
    ref = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    zero = (re == 0) & (im == 0)
    err = np.abs(got - ref)[~zero]   # (a zero product is +0 by definition, where atan2 says +-pi for re = -0: asserted below)
    print("fm_phase: largest error", err.max(), "rad =", err.max() / BOUND, "of the bound")
    assert err.max() <= BOUND


def test_phase_is_odd_in_im_to_the_bit(pairs):
    re, im = pairs
    nz = im != 0
    a = iq.phase(re[nz], im[nz])
    b = iq.phase(re[nz], -im[nz])
    assert np.array_equal(_u32(b), _u32(a) ^ np.uint32(0x80000000))


def test_phase_of_a_zero_product_is_plus_zero():
    z = np.array(list(itertools.product([0.0, -0.0], [0.0, -0.0])), dtype=np.float32)
    assert np.array_equal(_u32(iq.phase(z[:, 0], z[:, 1])), np.zeros(4, dtype=np.uint32))


def test_cross_is_four_products_and_two_sums_rounded_apart():
    rng = np.random.default_rng(6081)
    n = 200_000
    f32 = np.float32
    ints = [rng.integers(-32768, 32768, n).astype(np.int16).astype(f32) for _ in range(4)]
    flts = [(10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)).astype(f32) for _ in range(4)]
    for i, q, pi, pq in (ints, flts):
        re, im = iq.cross(i, q, pi, pq)
        a, b, c, d = (i * pi).astype(f32), (q * pq).astype(f32), (q * pi).astype(f32), (i * pq).astype(f32)
        assert np.array_equal(_u32(re), _u32((a + b).astype(f32))) and np.array_equal(_u32(im), _u32((c - d).astype(f32)))


def test_discriminate_is_gain_times_phase_of_cross():
    rng = np.random.default_rng(6082)
    x = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64) * np.float32(9000)
    for gain in (1.0, 5.0 / 3.0):
        out, carry = iq.discriminate(x, gain)
        prev = np.concatenate([np.zeros(1, dtype=np.complex64), x[:-1]])
        re, im = iq.cross(x.real, x.imag, prev.real, prev.imag)
        e = (np.float32(gain) * iq.phase(re, im)).astype(np.float32)
        assert np.array_equal(_u32(out), _u32(e)) and out[0] == 0 and not np.signbit(out[0])
        assert carry.tolist() == [x[-1].real, x[-1].imag]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------
KINDS = (0, 1, 2, 4)
CHANNELS = ((0.0, 0.0), (300.0, 0.0), (1500.0, 0.02))


NOISE_SEED = 1   # one fixed noise realisation.  (At sigma = 1500 the bare carrier of the tail is noise to the demodulator, and about one realisation in
# ten — seeds 4 and 8 of kind 2, 5 of kind 4 among 1..8 — grows one more low-cost frame there: with numpy's float32 arctan2 in place of fm_phase exactly as with
# fm_phase.  That is the signal's doing, not the discriminator's.)


def _good(recs):
    r = recs[recs["cost"] < 30]
    return [(int(t), bytes(p)) for t, p in zip(r["frame_type"], r["payload"])]


@pytest.fixture(scope="module")
def basebands():
    out = {}
    for kind in KINDS:
        s = ol.generate(ol.gen_params(seed=1, kind=kind, lead_in=9600, n_frames=6, tail=4800))
        s.setflags(write=False)
        out[kind] = (s, _good(ol.demod(s)[0]))
    return out


@pytest.mark.parametrize("fmt", [iq.IQ_I16, iq.IQ_F32], ids=["i16", "f32"])
@pytest.mark.parametrize("chan", CHANNELS, ids=["clean", "sigma300", "sigma1500_cfo"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_discriminated_transmission_carries_the_basebands_frames(basebands, kind, chan, fmt):
    s, expect = basebands[kind]
    sigma, cfo = chan
    assert len(expect) >= 1
    x = iq.fm_modulate(s, sigma=sigma, cfo=cfo, fmt=fmt, seed=NOISE_SEED)
    y, _ = iq.discriminate(x, 1.0)
    got = _good(fl.demod(y)[0])
    assert len(got) >= 1 and got == expect, (kind, chan, len(got), len(expect))
    # the spectrum flipped: the exact negation, which the inverted receiver undoes
    yc, _ = iq.discriminate(iq.fm_modulate(s, sigma=sigma, cfo=cfo, fmt=fmt, seed=NOISE_SEED, conj=True), 1.0)
    assert _good(fl.demod(yc, invert=1)[0]) == expect, (kind, chan, "conjugated")
    if fmt == iq.IQ_F32:   # (complex64 conjugation is exact; int16 clips -32768)
        nz = yc != 0
        assert np.array_equal(_u32(yc[nz]), _u32(y[nz]) ^ np.uint32(0x80000000)) and np.array_equal(yc == 0, y == 0)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [iq.IQ_I16, iq.IQ_F32], ids=["i16", "f32"])
def test_blocks_with_the_carry_passed_on_equal_one_block(fmt):
    rng = np.random.default_rng(6083)
    s = rng.integers(-21504, 21505, 5000).astype(np.int16)
    x = iq.fm_modulate(s, sigma=200.0, cfo=0.01, fmt=fmt)
    whole, end = iq.discriminate(x, 1.25)
    cuts = np.cumsum([0, 1, 2, 255, 1024]).tolist() + [5000]
    parts, carry = [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, carry = iq.discriminate(x[a:b], 1.25, carry)
        parts.append(o)
    assert np.array_equal(_u32(np.concatenate(parts)), _u32(whole)) and np.array_equal(carry, end)
    # the carry zeroed in front of the third block: a fresh feed — its first output is +0, the rest is what it was
    o, _ = iq.discriminate(x[cuts[2]:cuts[3]], 1.25, None)
    assert _u32(o)[0] == 0 and whole[cuts[2]] != 0 and np.array_equal(_u32(o[1:]), _u32(parts[2][1:]))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_upload_iq", "m17hip_upload_iq_device", "m17hip_upload_iq_async", "m17hip_upload_iq_device_async", "m17hip_iq_bytes"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 608
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for name in ("upload_iq", "upload_iq_async", "upload_iq_device", "upload_iq_device_async", "iq_bytes"):
        assert callable(getattr(m17hip.Context, name))
    assert (m17hip.IQ_I16, m17hip.IQ_F32) == (1, 2) and m17hip.KERNELS["discriminate"] == 8


def test_null_context_is_refused_by_every_new_call():
    lib = m17hip.load_library()
    x = np.zeros(64, dtype=np.complex64)
    for name in NEW[:4]:
        for fmt in (1, 2):
            assert getattr(lib, name)(C.c_void_p(), ol._p(x), C.c_int(fmt), C.c_float(1.0), C.c_uint32(1), C.c_uint32(64), C.c_size_t(64)) == -1, name
    n = C.c_uint64(7)
    assert lib.m17hip_iq_bytes(C.c_void_p(), C.byref(n)) == -1


def test_python_refuses_what_is_no_iq():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the array is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    for bad in (np.zeros((2, 8), dtype=np.float32), np.zeros((2, 8), dtype=np.complex128), np.zeros((2, 8, 3), dtype=np.int16), np.zeros((2, 8), dtype=np.int16)[:, :1]):
        with pytest.raises(TypeError):
            ctx.upload_iq(bad)


# ---- 5: the example, on the host form of the demodulator class ----------------------------------------------------------------------------------
def test_example_takes_iq_where_it_took_floats(basebands):
    """examples/m17-demod-gpu --iq-i16 / --iq-f32 [--iq-gain G] on IQ prints what --float32 prints on the host form's floats (M17_DEMOD_DEVICE=cpu: the
    scalar demodulator; on the GPU path the same class hands the IQ to m17hip_upload_iq, tests/test_gpu_iq_input.py)."""
    exe = os.path.join(iq.ROOT, "examples", "m17-demod-gpu")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ, M17_DEMOD_DEVICE="cpu")
    s, _ = basebands[1]
    for fmt, flag in ((iq.IQ_I16, "--iq-i16"), (iq.IQ_F32, "--iq-f32")):
        x = iq.fm_modulate(s, sigma=300.0, fmt=fmt, seed=NOISE_SEED)
        y, _ = iq.discriminate(x, 2.0)
        got = subprocess.run([exe, flag, "--iq-gain", "2"], input=x.tobytes(), capture_output=True, env=env, check=True).stdout
        exp = subprocess.run([exe, "--float32"], input=y.tobytes(), capture_output=True, env=env, check=True).stdout
        assert got == exp and len(got.splitlines()) >= 6, flag
    assert subprocess.run([exe, "--iq-i16", "--float32"], input=b"", capture_output=True, env=env).returncode == 2
    assert subprocess.run([exe, "--iq-f32", "--iq-gain", "0"], input=b"", capture_output=True, env=env).returncode == 2
