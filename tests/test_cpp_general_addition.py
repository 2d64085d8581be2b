"""dlaf::general_addition / hermitian_complete of the C++ facade include/dlaf_mi355x/dlaf.hpp (local and
grid overloads): tests/cpp_api/test_general_addition_cpp.cpp is compiled with g++ (CPU: the header is
self-contained and links) and run on the GPU on one process, one addition and one completion per element type, against
loops in the program (small integers: equality)."""
import os
import subprocess

import pytest

from test_cpp_api import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_general_addition_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_general_addition_cpp"))


@pytest.mark.gpu
def test_cpp_general_addition_matches_loops():
    r = subprocess.run([build_cpp_test("test_general_addition_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_GENERAL_ADDITION_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
