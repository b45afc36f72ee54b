"""CPU-only: float32 baseband input (ABI 607, include/m17hip.h).  1: the float oracle (tests/cxx/f32_oracle.cpp: the oracle's demodulator stepped on
floats) equals the int16 oracle on float(double(s) / 41067.0), so it can be the yardstick of the GPU tests.  2: the conditions under which those tests
bite — floats off the int16 grid change what the demodulator reports, floats beyond +-32767 / 41067 are lost by a host that must round — asserted on the
oracle alone.  3: what the new calls promise without a GPU: the symbols, the version, the argument refusals."""
import ctypes as C

import numpy as np
import pytest

import f32_lib as fl
import m17hip
import oracle_lib as ol

KINDS = {"bert": 0, "stream": 1, "packet": 2}
# (the generator settings of tests/test_gpu_channel_polarity.py's chain case: every kind decodes under them)
KW = dict(n_frames=10, lead_in=3072, noise_sigma=500.0, tail_sigma=500.0, lead_sigma=40000.0, total=28800)


@pytest.fixture(scope="module")
def signals():
    out = {}
    for name, kind in KINDS.items():
        for inv in (0, 1):   # (an inverted transmitter for the inverted receiver: it decodes under its own polarity only)
            s = ol.generate(ol.gen_params(seed=6070 + kind, kind=kind, invert=inv, **KW))
            s.setflags(write=False)
            out[name, inv] = s
    return out


def _log_cap(n):
    return n // 384 + 2


def _same(a, b):
    return a.tobytes() == b.tobytes()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("kind", list(KINDS))
def test_float_oracle_equals_the_int16_oracle_on_the_int16_grid(signals, kind, invert):
    s = signals[kind, invert].copy()
    if invert:
        s[s == -32768] = -32767   # (the one sample whose int16 negation wraps: asserted separately below)
    x = fl.on_grid(s)
    recs, diag = ol.demod(s, invert=invert)
    frecs, fdiag = fl.demod(x, invert=invert)
    assert recs.size >= 1, kind
    assert _same(frecs, recs) and _same(fdiag, diag)
    log = ol.demod_diag_log(s, invert=invert, cap=_log_cap(s.size))
    flog = fl.diag_log(x, invert=invert, cap=_log_cap(s.size))
    assert log.size > 10 and _same(flog, log)


def test_minus_32768_wraps_in_int16_and_not_in_float():
    """Inverted, int16 -32768 stays -32768 (the reference negates in int16) while the float -32768 / 41067 becomes +32768 / 41067."""
    s = np.full(8, -32768, dtype=np.int16)
    assert np.array_equal(ol.scale(s, invert=1), ol.scale(s, invert=0))            # the wrap
    x = fl.on_grid(s)
    assert np.array_equal(x, ol.scale(s, invert=0))
    neg = -x                                                                         # what a float stream computes under invert
    assert (neg > 0).all() and np.array_equal(neg.view(np.uint32), x.view(np.uint32) ^ np.uint32(0x80000000))
    assert not np.array_equal(neg, ol.scale(s, invert=1))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_off_grid_floats_do_not_survive_rounding_and_change_the_diagnostics(signals, kind):
    s = signals[kind, 0]
    x = fl.off_grid(s, seed=11)
    assert fl.survives_round_trip(x).mean() < 0.01
    recs, _ = fl.demod(x)
    assert recs.size >= 1, kind
    log = fl.diag_log(x, cap=_log_cap(s.size))
    rounded = ol.demod_diag_log(fl.round_trip(x), cap=_log_cap(s.size))
    assert log.size > 10 and not _same(log, rounded)


@pytest.mark.parametrize("kind", list(KINDS))
def test_four_times_the_amplitude_decodes_as_float_and_is_lost_when_saturated(signals, kind):
    """Stream and packet frames are delivered only below a cost limit (and after an LSF): saturated, they are lost (12 -> 1 and 11 -> 0 here).  A BERT frame
    is delivered whatever it costs (M17FrameDecoder.h: no cost gate on that path), so its count cannot fall: what saturation costs it is in the Viterbi
    cost and the payload bits (cost sum 177 as float, 1267 saturated)."""
    s = signals[kind, 0]
    x4 = fl.times4(s)
    assert (np.abs(x4) > 32767.0 / 41067.0).mean() > 0.3
    r1, r4, rsat = fl.demod(fl.on_grid(s))[0], fl.demod(x4)[0], ol.demod(fl.round_trip(x4))[0]
    assert r1.size >= 1 and r4.size >= r1.size, (kind, r1.size, r4.size)
    if kind == "bert":
        assert rsat.size <= r1.size and rsat["cost"].sum() > 2 * r4["cost"].sum() and rsat["payload"].tobytes() != r4["payload"].tobytes()
    else:
        assert rsat.size < r1.size, (kind, r1.size, rsat.size)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------
NEW = ["m17hip_upload_f32", "m17hip_upload_f32_async", "m17hip_upload_f32_device", "m17hip_upload_f32_device_async", "m17hip_download_f32",
       "m17hip_input_format"]


def test_exports_version_and_bindings():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 607
    for name in NEW:
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    for name in ("download_f32", "input_format"):
        assert callable(getattr(m17hip.Context, name))
    assert (m17hip.FORMAT_I16, m17hip.FORMAT_F32) == (1, 2)


def test_null_context_is_refused_by_every_new_call():
    lib = m17hip.load_library()
    x = np.zeros(64, dtype=np.float32)
    for name in NEW[:5]:
        assert getattr(lib, name)(C.c_void_p(), ol._p(x), C.c_uint32(1), C.c_uint32(64), C.c_size_t(64)) == -1, name
    assert lib.m17hip_input_format(C.c_void_p(), None, None) == -1


def test_python_refuses_other_dtypes_for_the_staging_calls():
    ctx = m17hip.Context.__new__(m17hip.Context)   # (no library call is made before the dtype is looked at)
    ctx.lib, ctx.h = m17hip.load_library(), C.c_void_p()
    for dt in (np.float64, np.int32, np.uint16):
        with pytest.raises(TypeError):
            ctx.upload_async(0, 1, 64, dtype=dt)
    assert ctx._by_dtype("_async", np.float32) is not None and ctx._by_dtype("_device", "int16") is not None
