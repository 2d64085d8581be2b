"""The non-terminating parts of the C API's argument checks (csrc/host/api_checks.hpp: the letter sets, the source
process inside the grid, the names a ScaLAPACK prologue composes for its messages) swept on the CPU by a stand-alone
host program (tests/api_checks/sweep.cpp) against a brute-force model the program writes from their definitions.  The
same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  The terminating
checks are pinned through the library by tests/test_c_api_preconditions.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "api_checks", "sweep.cpp")
INCS = [os.path.join(ROOT, "dla_future_amd", "csrc", "host"), os.path.join(ROOT, "include")]


def test_api_checks_sweep_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    builds = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    procs = {}
    for name, flags in builds.items():
        exe = str(tmp_path / f"sweep_{name}")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, *(f"-I{i}" for i in INCS), SRC, "-o", exe],
                       check=True, capture_output=True, text=True, timeout=300)
        procs[name] = subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, f"{name}: exit {p.returncode}\n{out}\n{err[-4000:]}"
        words = out.split()
        fields = dict(zip(words[0::2], (int(w) for w in words[1::2])))
        # 11 letter sets x 256 characters; 9 grids x 5 x 5 sources; 8 composed strings and the passing prologue
        assert fields == {"letters": 11 * 256, "sources": 9 * 25, "names": 9, "failures": 0}, out
