"""The eigenvalues-only functions (hermitian_eigenvalues, hermitian_generalized_eigenvalues) and the by-value overloads
(EigenvaluesValue) of the C++ facade include/dlaf_mi355x/dlaf.hpp: tests/cpp_api/test_eigenvalues_only_cpp.cpp is
compiled with g++ (CPU: the header is self-contained and links) and run on the GPU."""
import os
import subprocess

import pytest

from test_cpp_api import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_eigenvalues_only_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_eigenvalues_only_cpp"))


@pytest.mark.gpu
def test_cpp_eigenvalues_only_overloads():
    r = subprocess.run([build_cpp_test("test_eigenvalues_only_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_EIGENVALUES_ONLY_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
