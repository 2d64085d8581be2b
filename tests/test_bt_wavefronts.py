"""The wavefront schedule of bt_band_to_tridiagonal (csrc/host/bt_wavefronts.hpp: which reflector blocks run in one
batched launch, and in which order) swept on the CPU by a stand-alone host program (tests/bt_wavefronts/sweep.cpp)
against a model the program writes from the stage's definition: every block issued exactly once, its rows inside the
matrix, the blocks of a batch on disjoint rows, overlapping blocks in their one-by-one order and never in one batch, no
batch beyond the workspace bound nblk / 2 + 2.  b in {2, 3, 4, 5, 8, 16} with every n from 0 to 6 b + 3, and n = 20480
with b = 128; real and complex.  The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer
(host code only).  What the stage computes with this schedule is compared on the GPU
(tests/test_gpu_band_to_tridiag.py, tests/test_gpu_eigensolver.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "bt_wavefronts", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "host")


def test_bt_wavefronts_sweep_plain_and_sanitized(tmp_path):
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
        # 2 x (sum over b of 6 b + 4) + 2 cases; the two large ones alone hold 2 x 12 880 blocks in more than 600 batches
        assert fields["cases"] == 2 * (6 * 38 + 6 * 4) + 2, out
        assert fields["blocks"] > 25000 and fields["batches"] > 2000 and fields["failures"] == 0, out
