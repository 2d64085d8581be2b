"""CPU tests of the preconditions of the weighted Hermitian rank-k update and of the functions of a Hermitian matrix
(csrc/host/api_checks.hpp: require_weighted_rank_update, require_hermitian_function, require_power_threshold), in the style
of test_herk_preconditions.py: each case changes one argument of an otherwise valid n = 6, k = 4 call with block 2 and
expects the routine's message on stderr before the GPU is touched (the subprocesses run with the GPU hidden).  The
refusals that need a resident matrix are in tests/test_gpu_weighted_rank_update.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


SINGLE = "g = d.Grid.single()\n"
HOST_2X2 = "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)\n"
PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor, WEIGHTS_FN_D\n"
           "L = lib()\n"
           "a = np.ones((6, 4), order='F'); c = np.zeros((6, 6), order='F'); w = np.zeros(6); dw = np.ones(4)\n"
           "za = a.astype(np.complex128); zc = c.astype(np.complex128)\n"
           "al = np.array([1.0]); be = np.array([0.0])\n"
           "da = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "dc = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
           "uplo = b'L'; trans = b'N'; dptr = dw.ctypes.data; thr = 0.0\n"
           "fn = WEIGHTS_FN_D(lambda n, w, b, e, g, u: None)\n"
           "idx = np.array([0, 6], dtype=np.int64); val = np.array([0.0, 1.0]); iptr = None; vptr = None\n"
           "ctx = None\n")
CALLS = {
    "wherk": "r = L.dlaf_mi355x_hermitian_weighted_rank_k_update_d(g.context, uplo, trans, al.ctypes.data, a.ctypes.data, da, "
             "dptr, be.ctypes.data, c.ctypes.data, dc)",
    "zwherk": "r = L.dlaf_mi355x_hermitian_weighted_rank_k_update_z(g.context, uplo, trans, al.ctypes.data, za.ctypes.data, da, "
              "dptr, be.ctypes.data, zc.ctypes.data, dc)",
    "power": "r = L.dlaf_mi355x_hermitian_power_d(g.context, uplo, c.ctypes.data, dc, w.ctypes.data, -0.5, thr, None)",
    "function": "r = L.dlaf_mi355x_hermitian_function_d(g.context, uplo, c.ctypes.data, dc, w.ctypes.data, fn, None, iptr, "
                "vptr, None)",
}
W = "hermitian weighted rank-k update: "
F = "hermitian function: "
P = "hermitian power: "


def _terminates(grid, entry, mutate, needle):
    r = _run(PRELUDE + grid + f"{mutate}\n" + CALLS[entry] + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    for part in ((needle,) if isinstance(needle, str) else needle):
        assert part in r.stderr, (part, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("entry,mutate,needle", [
    ("wherk", "uplo = b'Q'", W + "bad uplo/trans 'Q' 'N'"),
    ("wherk", "trans = b'x'", W + "bad uplo/trans 'L' 'x'"),
    ("zwherk", "trans = b'T'; da.m, da.n = 4, 6", W + "trans 'T' on a complex type"),
    ("wherk", "dc.n = 5", W + "C must be square (6 x 5)"),
    ("wherk", "da.m = 5", W + "A is 5 x 4 (trans 'N'), C is 6 x 6"),
    ("wherk", "trans = b'C'", W + "A is 6 x 4 (trans 'C'), C is 6 x 6"),
    ("wherk", "da.mb = 3", W + "the operands need one square block (A 3 x 2, C 2 x 2)"),
    ("wherk", "dc.mb = dc.nb = 3", W + "the operands need one square block (A 2 x 2, C 3 x 3)"),
    ("wherk", "da.jsrc = 1", W + "source rank (0,1) outside the 1 x 1 grid"),
    ("wherk", "dc.i = 1", W + "sub-matrices are not supported"),
    ("wherk", "dptr = None", W + "the weights d are null (k = 4, alpha != 0)"),
    ("zwherk", "dptr = None", W + "the weights d are null (k = 4, alpha != 0)"),
    ("power", "thr = -1.0", P + "threshold -1 < 0"),
    ("power", "uplo = b'U'", P + "uplo = U is not implemented"),
    ("power", "dc.n = 5", P + "the matrix must be square (6 x 5)"),
    ("function", "iptr = idx.ctypes.data; vptr = val.ctypes.data", F + "two selections at once"),
    ("function", "idx[1] = 7; iptr = idx.ctypes.data", F),
    ("function", "dc.mb = 3", F + "the matrix needs a square block (3 x 2)"),
    ("function", "dc.j = 1", F + "sub-matrices are not supported"),
])
def test_preconditions_terminate(entry, mutate, needle):
    _terminates(SINGLE, entry, mutate, needle)


@pytest.mark.parametrize("entry,mutate,needle", [
    ("wherk", "da.isrc = 1", W + "A must start on C's process row (source row 1 vs 0)"),
    ("wherk", "dc.isrc = 2", W + "source rank (2,0) outside the 2 x 2 grid"),
    ("wherk", "trans = b'C'; da.m, da.n = 4, 6", W + "trans 'C' on a 2 x 2 grid: only 'N' is built on more than one process"),
    ("wherk", "trans = b'T'; da.m, da.n = 4, 6", W + "trans 'T' on a 2 x 2 grid"),
    ("function", "dc.jsrc = 2", F + "source rank (0,2) outside the 2 x 2 grid"),
])
def test_grid_preconditions_terminate(entry, mutate, needle):
    """On a 2 x 2 host grid (no broadcast is ever made) the alignment rule and the refusal of trans C / T fire."""
    _terminates(HOST_2X2, entry, mutate, needle)


def test_empty_and_quick_return_without_a_gpu():
    """n = 0 returns, and so does alpha = 0 / k = 0 with beta = 1 (d null allowed), before the GPU is touched; C keeps its
    bits; a function of the 0 x 0 matrix returns 0 as well"""
    r = _run(PRELUDE + SINGLE + "da.m = dc.m = dc.n = 0\n" + CALLS["wherk"] + "\nr1 = r\n" + CALLS["power"] + "\nr4 = r\n"
             "da.m = dc.m = dc.n = 6; be[0] = 1.0; al[0] = 0.0; c[:] = np.nan; a[:] = np.nan; dptr = None\n" + CALLS["wherk"] +
             "\nr2 = r\nal[0] = 1.0; da.n = 0\n" + CALLS["wherk"] + "\nprint('codes', r1, r4, r2, r, int(np.isnan(c).all()))")
    assert r.returncode == 0 and r.stdout.split() == ["codes", "0", "0", "0", "0", "1"], (r.stdout, r.stderr[-800:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]
