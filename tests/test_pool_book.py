"""The bookkeeping of the workspace pool (csrc/host/pool_book.hpp: which idle block a request gets, which blocks leave
when the idle bytes pass the cap, the cap from the text of DLAF_MI355X_POOL_GB) swept on the CPU by a stand-alone host
program (tests/pool_book/sweep.cpp) with fake pointers against a brute-force model the program writes from the pool's
rules.  The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  What
the pool asks of the driver (pool.cpp) runs in every GPU test of the eigensolver."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pool_book", "sweep.cpp")
INCS = [os.path.join(ROOT, "dla_future_amd", "csrc", "host")]


def test_pool_book_sweep_plain_and_sanitized(tmp_path):
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
        # 20 seeds x (3000 requests / give-backs + the closing release of everything idle); the directed expectations:
        # reuse window 4, threshold 4, cap 0 3, first-in-first-out 2 calls x 4, eviction 5, unknown pointers 3; the cap
        # from unset, 0, 0.5, 1.5, 64, a negative number and a word
        assert fields == {"steps": 20 * (3000 + 1), "directed": 4 + 4 + 3 + 2 * 4 + 5 + 3, "caps": 7, "failures": 0}, out
