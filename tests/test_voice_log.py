"""CPU-only: the voice consumer's rules (include/m17hip.h, ABI 606) as tests/voice_log.py restates them — every rule on hand-made record lists, then
on the oracle's records of one clean stream transmission — and what the new calls promise without a GPU: symbols, version, bindings, the refusal
of a NULL context, and a C++ host of BatchedDemodulator::enable_voice / voice / calls that builds against the mirror headers."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np

import m17hip
import oracle_lib as ol
import tx_build as tb
import voice_log as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSF_A = m17hip.make_lsf("W1AW/P", "SP5WWP-9", 0x0005, b"voice")
LSF_B = m17hip.make_lsf("", "N0CALL", 0x0005)
NEW = ("m17hip_voice_fetch", "m17hip_voice_device", "m17hip_calls_fetch", "m17hip_voice_feed")


def rec(ftype, pos, cost=0, payload=b""):
    r = np.zeros((), dtype=m17hip.FRAME_REC)
    r["frame_type"], r["sample_pos"], r["cost"] = ftype, pos, cost
    r["payload"] = np.frombuffer(bytes(payload).ljust(32, b"\0"), dtype=np.uint8)
    return r


def lsf(pos, body=LSF_A, cost=0):
    return rec(vl.FT_LSF, pos, cost, body)


def voice(pos, fn, cost=0, eos=False, fill=None):
    body = bytes([(fn + 7 * k) & 0xFF for k in range(16)]) if fill is None else bytes([fill]) * 16
    return rec(vl.FT_STREAM, pos, cost, m17hip.stream_row(fn, body, last=eos)[:18])


def call_tuple(c):
    return tuple(int(c[f]) for f in ("seq", "start_pos", "end_pos", "cost_sum", "frames", "blanked", "lost", "has_lsf", "close"))


# ---- the restatement, rule by rule ---------------------------------------------------------------------------------------------------------------
def test_eos_is_accepted_below_cost_70_only():
    for cost, closes in ((69, True), (70, False)):
        log = vl.VoiceLog()
        audio, marks, calls = log.feed([lsf(100), voice(2020, 0, 5), voice(3940, 1, cost, eos=True)])
        assert marks.tolist() == [vl.MARK_FIRST, vl.MARK_EOS if closes else 0], cost
        assert bytes(audio[1]) == bytes(voice(0, 1)["payload"][2:18])
        if closes:
            assert [call_tuple(c) for c in calls] == [(0, 100, 3940, 5 + cost, 2, 0, 0, 1, vl.CLOSE_EOS)] and log.call is None and log.seq == 1
            assert bytes(calls[0]["lsf"]) == LSF_A
        else:
            assert calls.size == 0 and log.call["frames"] == 2 and log.seq == 0


def test_blanking_starts_above_cost_80():
    log = vl.VoiceLog()
    _, marks, _ = log.feed([lsf(0), voice(1920, 0, 80), voice(3840, 1, 81), voice(5760, 2, 1000)])
    assert marks.tolist() == [vl.MARK_FIRST, vl.MARK_BLANK, vl.MARK_BLANK]
    assert (log.call["blanked"], log.call["cost_sum"], log.call["frames"]) == (2, 1161, 3)


def test_a_blanked_frame_with_the_eos_bit_does_not_close():
    log = vl.VoiceLog()
    _, marks, calls = log.feed([voice(0, 0), voice(1920, 1, 200, eos=True)])
    assert marks.tolist() == [vl.MARK_FIRST, vl.MARK_BLANK] and calls.size == 0 and log.call is not None


def test_frame_number_gap_and_wrap():
    log = vl.VoiceLog()
    _, marks, _ = log.feed([lsf(0), voice(1, 10), voice(2, 11), voice(3, 15), voice(4, 16)])          # 12, 13, 14 lost: a gap of 3
    assert marks.tolist() == [vl.MARK_FIRST, 0, vl.MARK_GAP, 0] and log.call["lost"] == 3
    _, marks, _ = log.feed([voice(5, 0x7FFE), voice(6, 0x7FFF), voice(7, 0), voice(8, 1)])             # ... then 0x7fff -> 0 is no gap
    assert marks.tolist() == [vl.MARK_GAP, 0, 0, 0] and log.call["lost"] == 3 + (0x7FFE - 16 - 1)
    _, marks, _ = log.feed([voice(9, 1), voice(10, 0)])                                               # a repeat, a step back
    assert marks.tolist() == [vl.MARK_GAP, vl.MARK_GAP]
    assert log.call["lost"] == (3 + 0x7FFE - 17 + 0x7FFF + 0x7FFE) & 0xFFFFFFFF
    first = vl.VoiceLog()
    _, marks, _ = first.feed([voice(0, 4000)])                                                        # a first frame has no predecessor
    assert marks.tolist() == [vl.MARK_FIRST] and first.call["lost"] == 0


def test_an_lsf_closes_the_open_call_and_opens_the_next():
    log = vl.VoiceLog(channel=9)
    _, _, calls = log.feed([lsf(50, LSF_A), voice(2000, 0, 3), voice(4000, 1, 4), lsf(9000, LSF_B), lsf(9500, LSF_A)])
    assert [call_tuple(c) for c in calls] == [(0, 50, 4000, 7, 2, 0, 0, 1, vl.CLOSE_LSF), (1, 9000, 9000, 0, 0, 0, 0, 1, vl.CLOSE_LSF)]
    assert bytes(calls[0]["lsf"]) == LSF_A and bytes(calls[1]["lsf"]) == LSF_B and calls["channel"].tolist() == [9, 9]
    assert log.call["lsf"] == LSF_A and log.call["start_pos"] == 9500 and log.seq == 2


def test_a_stream_record_with_no_call_open_opens_one_without_lsf():
    log = vl.VoiceLog()
    _, marks, calls = log.feed([voice(700, 33, 2), voice(2620, 34, 60, eos=True), voice(4540, 35, 90), lsf(9000)])
    assert marks.tolist() == [vl.MARK_FIRST, vl.MARK_EOS, vl.MARK_FIRST | vl.MARK_BLANK]
    assert [call_tuple(c) for c in calls] == [(0, 700, 2620, 62, 2, 0, 0, 0, vl.CLOSE_EOS), (1, 4540, 4540, 90, 1, 1, 0, 0, vl.CLOSE_LSF)]
    assert bytes(calls[0]["lsf"]) == bytes(30)


def test_other_frame_types_are_ignored_and_state_carries_between_feeds():
    whole, parts = vl.VoiceLog(), vl.VoiceLog()
    seq = [lsf(0), rec(1, 10, 0, b"\x01" * 6), voice(1920, 0, 1), rec(5, 2000, 99, b"\xff" * 25), rec(3, 2100, 0, b"\x02" * 26), voice(3840, 1, 2),
           rec(4, 4000), voice(5760, 2, 3, eos=True)]
    a, m, c = whole.feed(seq)
    assert m.tolist() == [vl.MARK_FIRST, 0, vl.MARK_EOS] and call_tuple(c[0]) == (0, 0, 5760, 6, 3, 0, 0, 1, vl.CLOSE_EOS)
    got = [parts.feed(seq[:3]), parts.feed(seq[3:4]), parts.feed(seq[4:])]
    assert np.array_equal(np.concatenate([g[0] for g in got]), a) and np.concatenate([g[1] for g in got]).tolist() == m.tolist()
    assert [g[2].size for g in got] == [0, 0, 1] and got[2][2].tobytes() == c.tobytes()
    parts.reset()
    assert parts.call is None and parts.seq == 0


def test_the_bank_orders_calls_by_channel_and_seq():
    bank = vl.VoiceBank(3, channel_base=40)
    audio, marks, counts, calls = bank.feed([[voice(0, 0, eos=True), voice(1, 0, eos=True)], [], [lsf(5), lsf(6)]])
    assert counts.tolist() == [2, 0, 0] and audio.shape == (3, 2, 16) and marks.shape == (3, 2)
    assert list(zip(calls["channel"].tolist(), calls["seq"].tolist())) == [(40, 0), (40, 1), (42, 0)]


# ---- the oracle's records of one clean transmission ---------------------------------------------------------------------------------------------
def test_one_clean_transmission_is_one_call():
    rng = np.random.default_rng(606)
    rows = [m17hip.stream_row(i, rng.integers(0, 256, 16, dtype=np.uint8), last=i == 5) for i in range(6)]
    p = ol.gen_params(seed=12, kind=tb.STREAM, n_frames=6, lead_in=2688, phase=3, tail=6000, noise_sigma=0.0)
    p.total = ol.generate(p).size
    recs, _ = ol.demod(tb.burst(p, tb.STREAM, LSF_A, rows))
    audio, marks, calls = vl.VoiceLog().feed(recs)
    assert calls.size == 1
    c = calls[0]
    assert (int(c["frames"]), int(c["lost"]), int(c["close"]), int(c["has_lsf"]), int(c["blanked"])) == (6, 0, vl.CLOSE_EOS, 1, 0)
    assert bytes(c["lsf"]) == LSF_A
    assert [bytes(a) for a in audio[:6]] == [r[2:18] for r in rows]
    assert marks[:6].tolist() == [vl.MARK_FIRST, 0, 0, 0, 0, vl.MARK_EOS]
    voice_pos = recs["sample_pos"][recs["frame_type"] == vl.FT_STREAM]
    assert int(c["start_pos"]) == int(recs["sample_pos"][recs["frame_type"] == vl.FT_LSF][0]) and int(c["end_pos"]) == int(voice_pos[5])


# ---- the ABI without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_bound():
    lib = m17hip.load_library()
    assert lib.m17hip_version() >= 606
    hdr = open(os.path.join(ROOT, "include", "m17hip.h")).read()
    exported = re.findall(r"global:\s*([^;]+);", open(os.path.join(ROOT, "m17-cxx-demod_amd", "csrc", "m17hip.map")).read())
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported), name
        assert hasattr(lib, name) and name in m17hip.EXPORTS, name
    assert "typedef struct m17_call_rec {" in hdr and "M17HIP_CALLS_PER_CHANNEL(room)" in hdr
    for method in ("voice", "voice_device", "calls", "voice_feed"):
        assert callable(getattr(m17hip.Context, method)), method
    assert m17hip.CALL_REC == vl.CALL_REC and m17hip.CALL_REC.itemsize == 72 and m17hip.KERNELS["voice"] == 7
    assert (m17hip.MARK_BLANK, m17hip.MARK_EOS, m17hip.MARK_FIRST, m17hip.MARK_GAP) == (vl.MARK_BLANK, vl.MARK_EOS, vl.MARK_FIRST, vl.MARK_GAP)
    macro = re.search(r"#define M17HIP_CALLS_PER_CHANNEL\(room\) \(\(room\) / (\d+)u \+ (\d+)u\)", hdr)
    assert macro and all(m17hip.calls_per_channel(r) == r // int(macro.group(1)) + int(macro.group(2)) for r in (1, 7, 8, 150, 65536))
    wrapper = open(os.path.join(ROOT, "m17-cxx-demod_amd", "include", "m17cxx", "BatchedDemodulator.h")).read()
    assert "m17hip_voice_fetch(ctx_" in wrapper and "m17hip_calls_fetch(ctx_" in wrapper and "m17hip_tune(ctx_, 34" in wrapper


def test_null_context_is_an_argument_error():
    lib = m17hip.load_library()
    buf = np.zeros(64 * 17, dtype=np.uint8)
    counts = np.zeros(4, dtype=np.uint32)
    recs = np.zeros((1, 4), dtype=m17hip.FRAME_REC)
    calls = np.zeros(4, dtype=m17hip.CALL_REC)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = C.c_uint32(0)
    assert lib.m17hip_voice_fetch(C.c_void_p(), p(buf), p(buf), p(counts), C.c_uint32(1), C.c_uint32(4)) == -1
    ptrs = [C.c_void_p() for _ in range(3)]
    assert lib.m17hip_voice_device(C.c_void_p(), C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]), C.byref(n)) == -1
    assert lib.m17hip_calls_fetch(C.c_void_p(), p(calls), C.c_uint32(4), C.byref(n)) == -1
    assert lib.m17hip_voice_feed(C.c_void_p(), p(recs), p(counts), C.c_uint32(1), C.c_uint32(4)) == -1


def build_cxx_driver(out_dir):
    """tests/cxx/voice_check.cpp, a host that calls BatchedDemodulator::enable_voice / voice / calls, built against the mirror headers and the library."""
    pkg = os.path.join(ROOT, "m17-cxx-demod_amd")
    exe = os.path.join(str(out_dir), "voice_check")
    subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(pkg, "include", "m17cxx"),
                    os.path.join(ROOT, "tests", "cxx", "voice_check.cpp"), "-L", pkg, "-lm17hip", "-L/opt/rocm/lib", "-Wl,-rpath," + pkg,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_the_cxx_wrapper_builds_and_refuses_a_bad_command_line(tmp_path):
    exe = build_cxx_driver(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2     # (usage: nothing of the GPU is touched)
    assert subprocess.run([exe, "x.i16", "4", "100", "0"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "x.i16", "0", "100", "8"], capture_output=True).returncode == 2
