"""The partial-spectrum overloads of the C++ facade include/dlaf_mi355x/dlaf.hpp (hermitian_eigensolver and
hermitian_generalized_eigensolver with an eigenvalue index range appended): tests/cpp_api/test_partial_spectrum_cpp.cpp
is compiled with g++ (CPU: the header is self-contained and links) and run on the GPU."""
import os
import subprocess

import pytest

from test_cpp_api import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_partial_spectrum_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_partial_spectrum_cpp"))


@pytest.mark.gpu
def test_cpp_partial_spectrum_overloads():
    r = subprocess.run([build_cpp_test("test_partial_spectrum_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_PARTIAL_SPECTRUM_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
