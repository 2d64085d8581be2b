"""The address arithmetic of the direct-to-LDS K loop (csrc/device/glds_addr.hpp: the slab an iteration loads, the
wave's slab base, the step from piece to piece, the 32-bit lane offset) swept on the CPU by a stand-alone host program
(tests/glds_addr/sweep.cpp) against the closed form (k0 + column) ld + row: both operands, every wave, piece and lane,
every slab of K = BK, 2 BK, 3 BK and 128 BK, every start slab with wrap-around, one and two segments, leading dimensions
up to 2^31 elements.  The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code
only).  What the loop computes with these addresses is compared on the GPU (tests/test_gpu_update_slab_bases.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "glds_addr", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")


def test_glds_addr_sweep_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    builds = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    procs = {}
    for name, flags in builds.items():
        exe = str(tmp_path / f"sweep_{name}")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True,
                       capture_output=True, text=True, timeout=300)
        procs[name] = subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, f"{name}: exit {p.returncode}\n{out}\n{err[-4000:]}"
        words = out.split()
        fields = dict(zip(words[0::2], (int(w) for w in words[1::2])))
        # every byte offset past 2^31 and past 2^32 is among the addresses compared
        assert fields["addresses"] > 10000000 and fields["slabs"] > 16000, out
        assert fields["past2^31"] > 1000000 and fields["past2^32"] > 1000000 and fields["failures"] == 0, out
