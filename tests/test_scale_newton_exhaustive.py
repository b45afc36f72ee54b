"""The scaling form K3 uses for every sample (csrc/m17_frontend_kernels.hpp dcd_scale2, two samples per packed instruction; the same
operations as core::scale_i16): q = s * RN(1/41067); r = fma(-q, 41067, s); x = fma(r, RN(1/41067), q).  Checked here for ALL 65 536
int16 values and both polarities against the oracle's scaling (the reference's double-precision division), with every operation
evaluated exactly and rounded once, as the hardware's IEEE multiply and fused multiply-add do.
(tests/test_oracle_kat.py::test_scale_identities_exhaustive checks this form on every seventh value.)"""
import numpy as np

import oracle_lib as ol


def _fma_f32(a, b, c):
    """RN_f32(a * b + c) for float32 arrays whose product a * b is exact in float64 (24 x 24 bits): the sum's rounding error is recovered
    (TwoSum) and folded in as a sticky bit (round to odd in float64), so the final rounding to float32 is the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    hi = p + c
    bb = hi - p
    lo = (p - (hi - bb)) + (c - bb)
    bits = hi.view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(lo > 0, np.inf, -np.inf)
    hi = np.where((lo != 0) & even, np.nextafter(hi, toward), hi)
    return hi.astype(np.float32)


def _newton_scale(s):
    fs = s.astype(np.float32)
    rcp = np.float32(1.0) / np.float32(41067.0)
    q = fs * rcp
    r = _fma_f32(-q, np.full_like(q, 41067.0), fs)
    return _fma_f32(r, np.full_like(q, rcp), q)


def test_fma_model_rounds_once():
    """The model above against exact rational arithmetic on values where a double rounding would show (a product that ends just
    beside a float32 midpoint of the sum)."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1.0 + 2.0 ** -12)
    c[::2] = rng.standard_normal(1000).astype(np.float32) * np.float32(2.0 ** 20)
    got = _fma_f32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        x = np.float32(float(exact))   # float(Fraction) and float32(double) are two roundings: take the best of the neighbours
        near = [x, np.nextafter(x, np.float32(np.inf), dtype=np.float32), np.nextafter(x, np.float32(-np.inf), dtype=np.float32)]
        best = min(near, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert np.float32(best).view(np.uint32) == got[i].view(np.uint32), i


def test_packed_scaling_form_equals_reference_for_every_int16():
    s = np.arange(-32768, 32768, dtype=np.int32)
    ref = ol.scale(s.astype(np.int16))
    assert np.array_equal(_newton_scale(s).view(np.uint32), ref.view(np.uint32))
    neg = (-s).astype(np.int16).astype(np.int32)              # the device negates in int16: -(-32768) wraps to -32768
    inv = ol.scale(s.astype(np.int16), invert=1)
    assert np.array_equal(_newton_scale(neg).view(np.uint32), inv.view(np.uint32))
