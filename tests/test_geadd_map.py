"""The index arithmetic of the addition / transposition kernel (csrc/device/geadd_map.hpp: the work units, which of them
run for a uplo mask and which elements they write, the vector / element decision, the source tile and element of a
destination element -- on one process and inside the class layout of a broadcast panel buffer --, the LDS image; the
definitions kernels_geadd.hip includes) swept on the CPU by a stand-alone host program (tests/geadd_map/sweep.cpp) that
walks every access of every thread as the kernel does, against brute-force models: every tile size from 1 to 170 with
ragged last tiles, every mask, rectangular shapes, grids up to 2 x 3 with every source process, and the read and write
sets of the in-place completion.  The same program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer (host code only).  What the kernel computes with these definitions is compared on the GPU
(tests/test_gpu_general_addition.py, tests/test_gpu_hermitian_complete.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "geadd_map", "sweep.cpp")
INCS = [os.path.join(ROOT, "dla_future_amd", "csrc", "device"), os.path.join(ROOT, "dla_future_amd", "csrc", "host")]


def test_geadd_map_sweep_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    builds = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    procs = {}
    for name, flags in builds.items():
        exe = str(tmp_path / f"sweep_{name}")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, *[f"-I{i}" for i in INCS], SRC, "-o", exe],
                       check=True, capture_output=True, text=True, timeout=300)
        procs[name] = subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, f"{name}: exit {p.returncode}\n{out}\n{err[-4000:]}"
        words = out.strip().splitlines()[-1].split()
        counts = dict(zip(words[0::2], map(int, words[1::2])))
        assert counts["failures"] == 0, out
        assert counts["elements"] > 100000000 and counts["units"] > 100000 and counts["panel_tiles"] > 5000 and \
            counts["inplace_units"] > 10000 and counts["decisions"] > 1000, out
        # the 16-byte path of every type: neither side of the LDS image more than 2-way conflicted
        lds = [ln for ln in out.splitlines() if ln.startswith("lds ")]
        assert len(lds) == 5, out
