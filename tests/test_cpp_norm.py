"""dlaf::auxiliary::max_norm (the reference's signature; General, Lower and Upper) and the dlaf::auxiliary::norm
overloads of the C++ facade include/dlaf_mi355x/dlaf.hpp: tests/cpp_api/test_norm_cpp.cpp is compiled with g++ (CPU: the
header is self-contained and links) and run on the GPU, where every overload must agree with the C entry it stands for at
n = 333, nb = 100, on host matrices and on a device-resident one."""
import os
import subprocess

import pytest

from test_cpp_api import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_norm_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_norm_cpp"))


@pytest.mark.gpu
def test_cpp_norm_overloads_agree_with_the_c_entries():
    r = subprocess.run([build_cpp_test("test_norm_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_NORM_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
