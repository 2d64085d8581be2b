"""The work-item map of the grouped update kernel (csrc/device/update_map.hpp: build_update_map, the host-side
construction launch_update calls) swept on the CPU by a stand-alone host program (tests/update_map/sweep.cpp): for pr,
pc in 1..4 with every (ri, ci), nt in 1..40, nb / BM in {1, 2, 3}, both BM / BN aspect ratios, sub-ranges and rect on
and off, every block the kernel's contract names lies in an enumerated patch, the work-item count is that of the
enumerated patches and the XCD remap is a permutation.  The same program runs once more under AddressSanitizer and
UndefinedBehaviorSanitizer (host code only).  The decode of a work item is the kernel's and is compared on the GPU
(tests/test_gpu_update_kernel.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "update_map", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")


def test_update_map_sweep_plain_and_sanitized(tmp_path):
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
        assert words[0] == "geometries" and int(words[1]) > 200000 and words[-2:] == ["failures", "0"], out
