"""CPU-only: the transmission builder of tests/tx_build.py (what tests/test_gpu_synth_tx.py holds m17hip_synth_tx_i16 against) pinned to the test
generator, what caller-supplied content shows on the oracle alone — FrameType::FULL_PACKET (M17FrameDecoder.h:113-136, 379-386) among it, which
no input of the suite produced before — and what the new call promises without a GPU."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import m17hip
import oracle_lib as ol
import spliced as sp
import tx_build as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the builder fed the generator's own truth is the generator -------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("n_frames", [1, 6, 7, 33])
@pytest.mark.parametrize("kind", [0, 1, 2, 4])
def test_builder_reproduces_the_generator(kind, n_frames, invert):
    p = ol.gen_params(seed=tb.channel_seed(605, 10 * kind + n_frames), kind=kind, n_frames=n_frames, lead_in=2688 if n_frames != 6 else 0,
                      phase=-1 if n_frames != 7 else 4, invert=invert, noise_sigma=300.0 if kind != 2 else 0.0, dc_offset=120.0 if kind == 1 else 0.0,
                      gain=0.7 if kind == 0 else 1.0, tail_sigma=100.0, tail=2500)
    p.total = ol.generate(p).size
    x, truth = ol.generate(p, with_truth=True)
    y = tb.burst(p, *tb.from_truth(kind, truth, n_frames))
    assert y.dtype == np.int16 and np.array_equal(x, y)


def test_builder_cuts_a_burst_longer_than_the_slab():
    p = ol.gen_params(seed=31, kind=1, n_frames=7, lead_in=100, noise_sigma=50.0)
    full, truth = ol.generate(p, with_truth=True)
    p.total = 5 * 1920 + 7
    assert np.array_equal(tb.burst(p, *tb.from_truth(1, truth, 7)), full[:p.total])


# ---- 2. the inputs bite ------------------------------------------------------------------------------------------------------------------------
def packet_rows(rng, n):
    """n packet frames of random bytes, numbered as apps/m17-mod.cpp numbers them: the last one flagged, with a byte count of 25."""
    return [bytes(rng.integers(0, 256, 25, dtype=np.uint8)) + bytes([0x80 | (25 << 2) if i == n - 1 else i << 2]) for i in range(n)]


def embedded(kind, lsf, rows, seed=11, sigma=200.0, phase=0):
    """The issue's surroundings: lead-in 2688, tail 6000, noise sigma 200."""
    p = ol.gen_params(seed=seed, kind=kind, n_frames=len(rows), lead_in=2688, phase=phase, tail=6000, noise_sigma=sigma)
    p.total = ol.generate(p).size
    return tb.burst(p, kind, lsf, rows), p.lead_in + phase


@pytest.mark.parametrize("type_field,frame_type", [(0x0004, sp.FT_FULL_PACKET), (0x0006, sp.FT_FULL_PACKET), (0x0000, sp.FT_FULL_PACKET),
                                                   (0x0002, sp.FT_BASIC_PACKET)])
def test_lsf_type_selects_the_packet_frame_type(type_field, frame_type):
    rows = packet_rows(np.random.default_rng(type_field + 1), 5)
    lsf = m17hip.make_lsf("", "N0CALL", type_field)
    recs, diag = ol.demod(embedded(tb.PACKET, lsf, rows)[0])
    assert recs["frame_type"].tolist() == [sp.FT_LSF] + [frame_type] * 5
    assert bytes(recs[0]["payload"][:30]) == lsf
    assert [bytes(r["payload"][:26]) for r in recs[1:]] == rows


def test_own_callsigns_and_stream_rows_come_back():
    rng = np.random.default_rng(17)
    lsf = m17hip.make_lsf("W1AW/P", "SP5WWP-9", 0x0005, b"meta")
    rows = [m17hip.stream_row(i, rng.integers(0, 256, 16, dtype=np.uint8), last=i == 8) for i in range(9)]
    recs, _ = ol.demod(embedded(tb.STREAM, lsf, rows, seed=12, phase=3)[0])
    assert recs[0]["frame_type"] == sp.FT_LSF and bytes(recs[0]["payload"][:30]) == lsf
    assert ol.decode_callsign(recs[0]["payload"][:6]).rstrip(b"\0") == b"W1AW/P"
    assert ol.decode_callsign(recs[0]["payload"][6:12]).rstrip(b"\0") == b"SP5WWP-9"
    got = [bytes(r["payload"][:18]) for r in recs if r["frame_type"] == sp.FT_STREAM]
    assert got[:9] == [r[:18] for r in rows]


def test_late_entry_assembles_the_supplied_lsf_from_lich():
    rng = np.random.default_rng(23)
    lsf = m17hip.make_lsf("AB1CDE", "K-./", 0x0005, bytes(range(1, 15)))
    rows = [m17hip.stream_row(i, rng.integers(0, 256, 16, dtype=np.uint8), last=i == 19) for i in range(20)]
    x, bs = embedded(tb.STREAM, lsf, rows, seed=13, phase=0)
    recs, _ = ol.demod(sp.late_entry(x, bs, 2, 0, 0))          # the preamble and the LSF frame are gone
    found = sp.assembled_lsf(recs)
    assert found and bytes(recs[found[0]]["payload"][:30]) == lsf
    assert ol.crc16(lsf) == 0


# ---- 3. the ABI without a GPU --------------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 605
    hdr = open(os.path.join(ROOT, "include", "m17hip.h")).read()
    assert re.search(r"\bint m17hip_synth_tx_i16\(", hdr) and "typedef struct m17_tx {" in hdr
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "m17-cxx-demod_amd", "csrc", "m17hip.map")).read())
    assert any(fnmatch.fnmatchcase("m17hip_synth_tx_i16", pat.strip()) for pat in exported)
    assert hasattr(lib, "m17hip_synth_tx_i16") and "m17hip_synth_tx_i16" in m17hip.EXPORTS
    assert callable(m17hip.Context.synth_tx) and m17hip.TX_DTYPE.itemsize == 16
    wrapper = open(os.path.join(ROOT, "m17-cxx-demod_amd", "include", "m17cxx", "BatchedDemodulator.h")).read()
    assert "m17hip_synth_tx_i16(ctx_" in wrapper


def test_null_arguments_are_argument_errors():
    lib = m17hip.load_library()
    base = ol.gen_params()
    tx = np.zeros(1, dtype=m17hip.TX_DTYPE)
    rows = np.zeros(32, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.m17hip_synth_tx_i16(C.c_void_p(), C.byref(base), p(tx), None, p(rows), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1920),
                                   C.c_uint32(0)) == -1


CALLSIGNS = ["", "N0CALL", "AB1CDE-9", "W1AW/P", "A.B-C/D12", "Z", "9", "SP5WWP", "ABCDEFGHI", "K-./"]


@pytest.mark.parametrize("call", CALLSIGNS)
def test_make_lsf_is_the_oracles_callsign_coding_and_crc(call):
    other = CALLSIGNS[(CALLSIGNS.index(call) + 3) % len(CALLSIGNS)]
    lsf = m17hip.make_lsf(call, other, 0x1234, b"\x01\x02")
    assert len(lsf) == 30
    assert lsf[:6] == (ol.encode_callsign(call) if call else b"\xff" * 6) and lsf[6:12] == ol.encode_callsign(other)
    assert m17hip.encode_callsign(call) == ol.encode_callsign(call)
    assert lsf[12:14] == b"\x12\x34" and lsf[14:28] == b"\x01\x02" + bytes(12)
    assert int.from_bytes(lsf[28:], "big") == ol.crc16(lsf[:28])
    row = m17hip.stream_row(0x1234, bytes(range(16)), last=True)
    assert len(row) == 32 and row[:2] == b"\x92\x34" and row[2:18] == bytes(range(16)) and row[18:] == bytes(14)
