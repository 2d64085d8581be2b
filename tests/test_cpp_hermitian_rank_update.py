"""dlaf::hermitian_rank_k_update / hermitian_rank_2k_update of the C++ facade include/dlaf_mi355x/dlaf.hpp (local and
grid overloads): tests/cpp_api/test_hermitian_rank_update_cpp.cpp is compiled with g++ (CPU: the header is
self-contained and links) and run on the GPU on one process, both updates, both uplo, NoTrans and ConjTrans, against
loop products in the program (small integers: equality)."""
import os
import subprocess

import pytest

from test_cpp_api import build_cpp_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_hermitian_rank_update_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_hermitian_rank_update_cpp"))


@pytest.mark.gpu
def test_cpp_hermitian_rank_update_matches_loop_products():
    r = subprocess.run([build_cpp_test("test_hermitian_rank_update_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_HERMITIAN_RANK_UPDATE_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
