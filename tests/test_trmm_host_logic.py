"""CPU tests of the triangular multiplication's host side (no GPU compute): the entry points are exported, and
every precondition of include/dlaf/multiplication/triangular.h terminates with its message before the GPU is
touched (the checks run on a box without one)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["dlaf_mi355x_triangular_multiplication_s", "dlaf_mi355x_triangular_multiplication_d",
           "dlaf_mi355x_triangular_multiplication_c", "dlaf_mi355x_triangular_multiplication_z",
           "dlaf_mi355x_pstrmm", "dlaf_mi355x_pdtrmm", "dlaf_mi355x_pctrmm", "dlaf_mi355x_pztrmm",
           "dlaf_mi355x_triangular_multiplication_device", "dlaf_mi355x_multiplication_profile"]


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_multiplication_entries_exported():
    import dla_future_amd as d
    from dla_future_amd.capi import SIGNATURES
    L = C.CDLL(d.lib_path())
    for name in ENTRIES:
        assert hasattr(L, name) and name in SIGNATURES, name
    for name in ("triangular_multiplication", "triangular_multiplication_device", "pxtrmm", "multiplication_profile"):
        assert callable(getattr(d, name)) and name in d.__all__, name


PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "a = np.eye(6, order='F'); b = np.ones((6, 4), order='F'); al = np.array([1.0])\n"
           "da = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6); db = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "side, uplo, op, diag = 'L', 'L', 'N', 'N'\n")


@pytest.mark.parametrize("mutate,needle", [
    ("side = 'X'", "triangular multiplication: bad side/uplo/op/diag"),
    ("uplo = 'Q'", "triangular multiplication: bad side/uplo/op/diag"),
    ("op = 'Z'", "triangular multiplication: bad side/uplo/op/diag"),
    ("diag = 'V'", "triangular multiplication: bad side/uplo/op/diag"),
    ("da.n = 5", "triangular multiplication: A must be square"),
    ("da.mb = 3", "triangular multiplication: A must be square"),
    ("db.m = 7", "triangular multiplication: A is 6 x 6, B is 7 x 4"),
    ("side = 'R'", "triangular multiplication: A is 6 x 6, B is 6 x 4 (side R)"),
    ("db.mb = 3", "triangular multiplication: B's blocks"),
    ("db.isrc = 3", "outside the 1 x 1 grid"),
    ("da.jsrc = 1", "outside the 1 x 1 grid"),
])
def test_triangular_multiplication_preconditions_terminate(mutate, needle):
    r = _run(PRELUDE + "g = d.Grid.single()\n" + f"{mutate}\n"
             "lib().dlaf_mi355x_triangular_multiplication_d(g.context, side.encode(), uplo.encode(), op.encode(), "
             "diag.encode(), al.ctypes.data, a.ctypes.data, da, b.ctypes.data, db)\n"
             "print('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and needle in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("side,mutate", [("L", "db.isrc = 1"), ("R", "da.jsrc = 1")])
def test_triangular_multiplication_source_process_terminates(side, mutate):
    """A and B must share the source process along the triangular dimension: a 2 x 2 host grid (no broadcast is
    ever made) with B's source row (side L) / A's source column (side R) moved."""
    r = _run(PRELUDE + "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)\n"
             f"side = '{side}'\n"
             "da = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
             "db = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6) if side == 'L' else DLAFDescriptor(4, 6, 2, 2, 0, 0, 0, 0, 6)\n"
             "b = np.ones((6, 6), order='F')\n"
             f"{mutate}\n"
             "lib().dlaf_mi355x_triangular_multiplication_d(g.context, side.encode(), uplo.encode(), op.encode(), "
             "diag.encode(), al.ctypes.data, a.ctypes.data, da, b.ctypes.data, db)\n"
             "print('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    assert "triangular multiplication: A and B must share the source process along the triangular dimension" in r.stderr, \
        r.stderr[-500:]
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


def test_pxtrmm_bad_descriptor_terminates():
    r = _run("import numpy as np, dla_future_amd as d\n"
             "g = d.Grid.single(); a = np.eye(4, order='F'); b = np.ones((4, 3), order='F')\n"
             "d.pxtrmm('L', 'L', 'N', 'N', 4, 3, 1.0, a, 1, 1, [1, g.context, 4, 4, 2, 2, 0, 0, 4], b, 2, 1, "
             "[1, g.context, 4, 3, 2, 2, 0, 0, 4])\n"
             "print('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and "ia, ja, ib, jb must be 1" in r.stderr, r.stderr[-500:]
