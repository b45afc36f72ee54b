"""CPU-only: what m17hip_set_channel_polarity (include/m17hip.h) promises without a GPU — the symbol, the version, the bindings, the refusal of
a NULL context, and that a C++ host calling BatchedDemodulator::set_channel_polarity builds against the mirror headers."""
import ctypes as C
import os
import subprocess

import numpy as np

import m17hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_an_argument_error():
    lib = m17hip.load_library()
    tab = np.array([0, 1], dtype=np.uint8)
    assert lib.m17hip_set_channel_polarity(C.c_void_p(), tab.ctypes.data_as(C.c_void_p), C.c_uint32(2)) == -1
    assert lib.m17hip_set_channel_polarity(C.c_void_p(), None, C.c_uint32(0)) == -1


def test_the_call_is_bound_everywhere():
    assert "m17hip_set_channel_polarity" in m17hip.EXPORTS and callable(getattr(m17hip.Context, "set_channel_polarity"))
    assert m17hip.load_library().m17hip_version() >= 604


def build_cxx_driver(out_dir):
    """tests/cxx/channel_polarity_check.cpp, a host that calls BatchedDemodulator::set_channel_polarity, built against the mirror headers and the library."""
    pkg = os.path.join(ROOT, "m17-cxx-demod_amd")
    exe = os.path.join(str(out_dir), "channel_polarity_check")
    subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-I", os.path.join(pkg, "include", "m17cxx"),
                    os.path.join(ROOT, "tests", "cxx", "channel_polarity_check.cpp"), "-L", pkg, "-lm17hip", "-L/opt/rocm/lib", "-Wl,-rpath," + pkg,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_the_cxx_wrapper_builds_and_refuses_a_bad_command_line(tmp_path):
    exe = build_cxx_driver(tmp_path)
    assert subprocess.run([exe], capture_output=True).returncode == 2     # (usage: nothing of the GPU is touched)
    assert subprocess.run([exe, "x.i16", "4", "100", "012x"], capture_output=True).returncode == 2
