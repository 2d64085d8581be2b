"""The kernel choice of the panel TRSM (csrc/device/trsm_path.hpp: trsm_path, the host function launch_trsm selects
through) swept on the CPU by a stand-alone host program (tests/trsm_path/sweep.cpp) over nb, last_rows, n, the alignment
of the three base pointers and of the strides, upper, the DLAF_MI355X_TRSM=strips switch and the four types: a row-owner
kernel only when every promise its comments rely on holds, the strips kernel otherwise.  The same program runs once
more under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  What the chosen kernels compute is
compared on the GPU (tests/test_gpu_trsm_kernel.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "trsm_path", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")


def test_trsm_path_sweep_plain_and_sanitized(tmp_path):
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
        assert words[:2] == ["argument", "sets"] and int(words[2]) > 1000000 and int(words[4]) > 1000 and \
            words[-2:] == ["failures", "0"], out
