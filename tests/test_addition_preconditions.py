"""CPU tests of the preconditions of general_addition and hermitian_complete (csrc/host/api_checks.hpp:
require_general_addition, require_hermitian_complete, behind the descriptor entries and the p? entries), in the style of
test_herk_preconditions.py: each case changes one argument of an otherwise valid 6 x 4 call with block 2 and expects the
routine's message on stderr before the GPU is touched (the subprocesses run with the GPU hidden).  The quick returns
(m = 0, n = 0, alpha = 0 with beta = 1) need no GPU either."""
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
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "L = lib()\n"
           "a = np.ones((6, 4), order='F'); c = np.zeros((6, 4), order='F'); s = np.ones((6, 6), order='F')\n"
           "al = np.array([1.0]); be = np.array([0.0])\n"
           "da = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6); dc = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "ds = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
           "uplo = b'A'; op = b'N'; kind = b'H'; ia = ja = ic = jc = 1; m = 6; n = 4\n"
           "ap = a.ctypes.data; cp = c.ctypes.data\n")
DESCS = ("ctx = g.context\n"
         "sa = (C.c_int * 9)(1, ctx, 6, 4, 2, 2, 0, 0, 6); sc = (C.c_int * 9)(1, ctx, 6, 4, 2, 2, 0, 0, 6)\n")
CALLS = {
    "add": "r = L.dlaf_mi355x_general_addition_d(ctx, uplo, op, al.ctypes.data, ap, da, be.ctypes.data, cp, dc)",
    "complete": "r = L.dlaf_mi355x_hermitian_complete_d(ctx, uplo, kind, s.ctypes.data, ds)",
    "pdgeadd": "r = L.dlaf_mi355x_pdgeadd(op, m, n, al.ctypes.data, ap, ia, ja, sa, be.ctypes.data, cp, ic, jc, sc)",
    "pdtradd": "r = L.dlaf_mi355x_pdtradd(uplo, op, m, n, al.ctypes.data, ap, ia, ja, sa, be.ctypes.data, cp, ic, jc, sc)",
    "pdtran": "r = L.dlaf_mi355x_pdtran(m, n, al.ctypes.data, ap, ia, ja, sa, be.ctypes.data, cp, ic, jc, sc)",
    "pdlacpy": "r = L.dlaf_mi355x_pdlacpy(uplo, m, n, ap, ia, ja, sa, cp, ic, jc, sc)",
}
GA = "general addition: "
HC = "hermitian complete: "


def _terminates(grid, entry, mutate, needle):
    r = _run(PRELUDE + grid + DESCS + f"{mutate}\n" + CALLS[entry] + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    for part in ((needle,) if isinstance(needle, str) else needle):
        assert part in r.stderr, (part, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("entry,mutate,needle", [
    ("add", "uplo = b'Q'", GA + "bad uplo/op 'Q' 'N'"),
    ("add", "op = b'x'", GA + "bad uplo/op 'A' 'x'"),
    ("add", "da.mb = 3", GA + "A and C need one square block (A 3 x 2, C 2 x 2)"),
    ("add", "dc.mb = dc.nb = 3", GA + "A and C need one square block (A 2 x 2, C 3 x 3)"),
    ("add", "da.m = 5", GA + "A is 5 x 4 (op 'N'), C is 6 x 4"),
    ("add", "op = b'T'", GA + "A is 6 x 4 (op 'T'), C is 6 x 4"),
    ("add", "da.i = 1", GA + "sub-matrices are not supported"),
    ("add", "dc.j = 2", GA + "sub-matrices are not supported"),
    ("add", "da.jsrc = 1", GA + "source rank (0,1) outside the 1 x 1 grid"),
    ("add", "op = b'T'; c = s; cp = ap = s.ctypes.data; da.n = dc.n = 6", GA + "A and C are the same matrix, which only op 'N' accepts"),
    ("add", "op = b'C'; c = s; cp = ap = s.ctypes.data; da.n = dc.n = 6", GA + "A and C are the same matrix, which only op 'N' accepts"),
    ("pdgeadd", "ic = 2", (GA, "ia, ja, ic, jc must be 1")),
    ("pdgeadd", "sc[0] = 2", (GA, "(dtype) must be 1")),
    ("pdgeadd", "sa[1] = ctx - 1", (GA, "A and C live on different contexts")),
    ("pdtradd", "uplo = b'A'", (GA, "uplo must be 'L' or 'U'")),
    ("pdtran", "ja = 3", (GA, "ia, ja, ic, jc must be 1")),
    ("pdlacpy", "jc = 0", (GA, "ia, ja, ic, jc must be 1")),
    ("complete", "uplo = b'A'", HC + "bad uplo/kind 'A' 'H'"),
    ("complete", "kind = b'T'", HC + "bad uplo/kind 'L' 'T'"),
    ("complete", "ds.n = 5", HC + "the matrix must be square (6 x 5)"),
    ("complete", "ds.mb = 3", HC + "the matrix needs a square block (3 x 2)"),
    ("complete", "ds.i = 2", HC + "sub-matrices are not supported"),
    ("complete", "ds.isrc = 1", HC + "source rank (1,0) outside the 1 x 1 grid"),
])
def test_addition_preconditions_terminate(entry, mutate, needle):
    if entry == "complete" and "uplo" not in mutate:
        mutate = "uplo = b'L'; " + mutate
    if entry == "pdtradd" and "uplo" not in mutate:
        mutate = "uplo = b'L'; " + mutate
    _terminates(SINGLE, entry, mutate, needle)


@pytest.mark.parametrize("entry,mutate,needle", [
    ("add", "da.isrc = 1", GA + "op 'N' needs A on C's source process (source 1,0 vs 0,0)"),
    ("add", "da.jsrc = 1; dc.isrc = 1", GA + "op 'N' needs A on C's source process (source 0,1 vs 1,0)"),
    ("add", "dc.isrc = 2", GA + "source rank (2,0) outside the 2 x 2 grid"),
    ("pdlacpy", "sa[6] = 1", GA + "op 'N' needs A on C's source process (source 1,0 vs 0,0)"),
    ("complete", "uplo = b'U'; ds.jsrc = 2", HC + "source rank (0,2) outside the 2 x 2 grid"),
])
def test_addition_grid_preconditions_terminate(entry, mutate, needle):
    """On a 2 x 2 host grid (no broadcast is ever made) the source rule of op N fires."""
    _terminates(HOST_2X2, entry, mutate, needle)


def test_addition_empty_and_quick_return_without_a_gpu():
    """m = 0 or n = 0 returns, and so does alpha = 0 with beta = 1, before the GPU is touched; C keeps its bits and the
    NaNs of A reach nothing"""
    r = _run(PRELUDE + SINGLE + DESCS + "da.m = dc.m = 0\n" + CALLS["add"] + "\nr1 = r\n"
             "da.m = dc.m = 6; da.n = dc.n = 0\n" + CALLS["add"] + "\nr2 = r\n"
             "da.n = dc.n = 4; be[0] = 1.0; al[0] = 0.0; c[:] = np.nan; a[:] = np.nan\n" + CALLS["add"] + "\nr3 = r\n"
             "ds.m = ds.n = 0; uplo = b'L'\n" + CALLS["complete"] + "\nr4 = r\n"
             "m = 0\n" + CALLS["pdlacpy"] + "\n"
             "print('codes', r1, r2, r3, r4, int(np.isnan(c).all()))")
    assert r.returncode == 0 and r.stdout.split() == ["codes", "0", "0", "0", "0", "1"], (r.stdout, r.stderr[-800:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]
