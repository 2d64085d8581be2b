"""The index arithmetic of the Hermitian rank-k / rank-2k update kernel (csrc/device/herk_map.hpp: which blocks run,
which elements are stored, which are diagonal, trans -> operand forms, panel offsets -- the definitions kernels_herk.hip
includes) swept on the CPU by a stand-alone host program (tests/herk_map/sweep.cpp) against brute-force models: every
tile size from 1 to 170 with ragged last tiles, both block shapes, grids up to 2 x 3 with every source process.  The
same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  What the kernel
computes with these definitions is compared on the GPU (tests/test_gpu_hermitian_rank_update.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "herk_map", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")


def test_herk_map_sweep_plain_and_sanitized(tmp_path):
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
        assert words[0] == "elements" and int(words[1]) > 10000000 and int(words[3]) > 10000 and int(words[5]) > 10000 and \
            words[-2:] == ["failures", "0"], out
