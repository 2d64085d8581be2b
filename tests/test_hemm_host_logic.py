"""CPU tests of the Hermitian multiplication's host side (no GPU compute): the entry points are exported, and every
precondition of include/dlaf/multiplication/hermitian.h (and of this build) terminates with its
`hermitian multiplication:` message before the GPU is touched (the checks run on a box without one)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ["dlaf_mi355x_hermitian_multiplication_s", "dlaf_mi355x_hermitian_multiplication_d",
           "dlaf_mi355x_hermitian_multiplication_c", "dlaf_mi355x_hermitian_multiplication_z",
           "dlaf_mi355x_pssymm", "dlaf_mi355x_pdsymm", "dlaf_mi355x_pchemm", "dlaf_mi355x_pzhemm",
           "dlaf_mi355x_hermitian_multiplication_device", "dlaf_mi355x_multiplication_profile"]


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


def test_hermitian_entries_exported():
    import dla_future_amd as d
    from dla_future_amd.capi import SIGNATURES
    L = C.CDLL(d.lib_path())
    for name in ENTRIES:
        assert hasattr(L, name) and name in SIGNATURES, name
    for name in ("hermitian_multiplication", "hermitian_multiplication_device", "pxhemm", "multiplication_profile"):
        assert callable(getattr(d, name)) and name in d.__all__, name


PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "a = np.eye(6, order='F'); b = np.ones((6, 4), order='F'); c = np.ones((6, 4), order='F')\n"
           "al = np.array([1.0]); be = np.array([0.5])\n"
           "da = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6); db = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "dc = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "side, uplo = 'L', 'L'\n")
CALL = ("lib().dlaf_mi355x_hermitian_multiplication_d(g.context, side.encode(), uplo.encode(), al.ctypes.data, "
        "a.ctypes.data, da, b.ctypes.data, db, be.ctypes.data, c.ctypes.data, dc)\n"
        "print('survived')")


def _check(r, needle):
    assert r.returncode != 0 and "survived" not in r.stdout and needle in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("mutate,needle", [
    ("side = 'X'", "hermitian multiplication: bad side/uplo"),
    ("uplo = 'Q'", "hermitian multiplication: bad side/uplo"),
    ("da.n = 5", "hermitian multiplication: A must be square"),
    ("da.mb = 3", "hermitian multiplication: A must be square"),
    ("db.m = 7; dc.m = 7", "hermitian multiplication: A is 6 x 6, B and C are 7 x 4 (side L)"),
    ("side = 'R'", "hermitian multiplication: A is 6 x 6, B and C are 6 x 4 (side R)"),
    ("db.n = 5", "hermitian multiplication: B (6 x 5, blocks 2 x 2) and C (6 x 4, blocks 2 x 2) differ"),
    ("db.nb = 3", "hermitian multiplication: B (6 x 4, blocks 2 x 3) and C (6 x 4, blocks 2 x 2) differ"),
    ("db.mb = 3; dc.mb = 3", "hermitian multiplication: the blocks of B and C (3 x 2) do not match A's"),
    ("da.i = 2", "hermitian multiplication: sub-matrices are not supported"),
    ("dc.isrc = 3", "hermitian multiplication: source rank (3,0) outside the 1 x 1 grid"),
    ("da.jsrc = 1", "hermitian multiplication: source rank (0,1) outside the 1 x 1 grid"),
])
def test_hermitian_multiplication_preconditions_terminate(mutate, needle):
    _check(_run(PRELUDE + "g = d.Grid.single()\n" + f"{mutate}\n" + CALL), needle)


@pytest.mark.parametrize("side,mutate,needle", [
    ("L", "db.isrc = 1; dc.isrc = 1", "hermitian multiplication: A must share the source process of B and C along"),
    ("R", "da.jsrc = 1", "hermitian multiplication: A must share the source process of B and C along"),
    ("L", "db.jsrc = 1", "hermitian multiplication: B and C must share the source process ((0,1) vs (0,0))"),
    ("R", "dc.isrc = 1", "hermitian multiplication: B and C must share the source process ((0,0) vs (1,0))"),
])
def test_hermitian_multiplication_source_process_terminates(side, mutate, needle):
    """A shares the source process of B and C along A's dimension, and B and C share theirs: a 2 x 2 host grid (no
    broadcast is ever made) with one source coordinate moved."""
    _check(_run(PRELUDE + "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)\n"
                f"side = '{side}'\n"
                "shape = (6, 6) if side == 'L' else (4, 6)\n"
                "db = DLAFDescriptor(shape[0], shape[1], 2, 2, 0, 0, 0, 0, 6)\n"
                "dc = DLAFDescriptor(shape[0], shape[1], 2, 2, 0, 0, 0, 0, 6)\n"
                "b = np.ones((6, 6), order='F'); c = np.ones((6, 6), order='F')\n"
                f"{mutate}\n" + CALL), needle)


def test_pxhemm_bad_descriptor_terminates():
    r = _run("import numpy as np, dla_future_amd as d\n"
             "g = d.Grid.single(); a = np.eye(4, order='F'); b = np.ones((4, 3), order='F'); c = np.ones((4, 3), order='F')\n"
             "d.pxhemm('L', 'L', 4, 3, 1.0, a, 2, 1, [1, g.context, 4, 4, 2, 2, 0, 0, 4], b, 1, 1, "
             "[1, g.context, 4, 3, 2, 2, 0, 0, 4], 0.0, c, 1, 1, [1, g.context, 4, 3, 2, 2, 0, 0, 4])\n"
             "print('survived')")
    _check(r, "hermitian multiplication: ia, ja, ib, jb, ic, jc must be 1")
