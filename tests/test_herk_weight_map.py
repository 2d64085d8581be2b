"""The weight index arithmetic of the weighted rank-k update (csrc/device/herk_map.hpp: herk_weight_slots / _k / _slot --
which real weight each register of the slab loader takes, the definitions kernels_herk.hip includes) swept on the CPU by a
stand-alone host program (tests/herk_weight_map/sweep.cpp) against the loader's own enumeration of (row, k), for the slab
shapes of all four element types and every loader mode.  The same program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer (host code only).  What the kernel computes with these definitions is pinned on the GPU by the
one-hot weights of tests/test_gpu_weighted_rank_update.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "herk_weight_map", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")


def test_herk_weight_map_sweep_plain_and_sanitized(tmp_path):
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
        assert words[0] == "registers" and int(words[1]) > 40000 and words[-2:] == ["failures", "0"], out
