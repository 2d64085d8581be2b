"""CPU tests of the preconditions of the Hermitian rank-k / rank-2k updates (csrc/host/api_checks.hpp:
require_rank_update, behind the descriptor entries, the p? entries and the resident ones), in the style of
test_gemm_preconditions.py: each case changes one argument of an otherwise valid n = 6, k = 4 call with block 2 and
expects the routine's message on stderr before the GPU is touched (the subprocesses run with the GPU hidden).  The
refusals that need a resident matrix (a stored triangle that is not uplo, operands of different contexts or element
types) are in tests/test_gpu_hermitian_rank_update.py."""
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
           "a = np.ones((6, 4), order='F'); b = np.ones((6, 4), order='F'); c = np.zeros((6, 6), order='F')\n"
           "za = a.astype(np.complex128); zc = c.astype(np.complex128); zal = np.array([1.0 + 0j])\n"
           "al = np.array([1.0]); be = np.array([0.0])\n"
           "da, db = (DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6) for _ in range(2))\n"
           "dc = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
           "uplo = b'L'; trans = b'N'; ia = ja = ib = jb = ic = jc = 1; n = 6; k = 4\n")
DESCS = ("ctx = g.context\n"
         "sa, sb = ((C.c_int * 9)(1, ctx, 6, 4, 2, 2, 0, 0, 6) for _ in range(2))\n"
         "sc = (C.c_int * 9)(1, ctx, 6, 6, 2, 2, 0, 0, 6)\n")
CALLS = {
    "herk": "r = L.dlaf_mi355x_hermitian_rank_k_update_d(ctx, uplo, trans, al.ctypes.data, a.ctypes.data, da, "
            "be.ctypes.data, c.ctypes.data, dc)",
    "zherk": "r = L.dlaf_mi355x_hermitian_rank_k_update_z(ctx, uplo, trans, al.ctypes.data, za.ctypes.data, da, "
             "be.ctypes.data, zc.ctypes.data, dc)",
    "her2k": "r = L.dlaf_mi355x_hermitian_rank_2k_update_d(ctx, uplo, trans, al.ctypes.data, a.ctypes.data, da, "
             "b.ctypes.data, db, be.ctypes.data, c.ctypes.data, dc)",
    "zher2k": "r = L.dlaf_mi355x_hermitian_rank_2k_update_z(ctx, uplo, trans, zal.ctypes.data, za.ctypes.data, da, "
              "za.ctypes.data, db, be.ctypes.data, zc.ctypes.data, dc)",
    "pdsyrk": "r = L.dlaf_mi355x_pdsyrk(uplo, trans, n, k, al.ctypes.data, a.ctypes.data, ia, ja, sa, be.ctypes.data, "
              "c.ctypes.data, ic, jc, sc)",
    "pdsyr2k": "r = L.dlaf_mi355x_pdsyr2k(uplo, trans, n, k, al.ctypes.data, a.ctypes.data, ia, ja, sa, b.ctypes.data, ib, "
               "jb, sb, be.ctypes.data, c.ctypes.data, ic, jc, sc)",
    "pzherk": "r = L.dlaf_mi355x_pzherk(uplo, trans, n, k, al.ctypes.data, za.ctypes.data, ia, ja, sa, be.ctypes.data, "
              "zc.ctypes.data, ic, jc, sc)",
}
K1 = "hermitian rank-k update: "
K2 = "hermitian rank-2k update: "


def _terminates(grid, entry, mutate, needle):
    r = _run(PRELUDE + grid + DESCS + f"{mutate}\n" + CALLS[entry] + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    for part in ((needle,) if isinstance(needle, str) else needle):
        assert part in r.stderr, (part, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("entry,mutate,needle", [
    ("herk", "uplo = b'Q'", K1 + "bad uplo/trans 'Q' 'N'"),
    ("herk", "trans = b'x'", K1 + "bad uplo/trans 'L' 'x'"),
    ("her2k", "trans = b'x'", K2 + "bad uplo/trans 'L' 'x'"),
    ("zherk", "trans = b'T'; da.m, da.n = 4, 6", K1 + "trans 'T' on a complex type"),
    ("zher2k", "trans = b'T'; da.m, da.n = 4, 6; db.m, db.n = 4, 6", K2 + "trans 'T' on a complex type"),
    ("pzherk", "trans = b't'", K1 + "trans 't' on a complex type"),
    ("herk", "dc.n = 5", K1 + "C must be square (6 x 5)"),
    ("herk", "da.m = 5", K1 + "A is 5 x 4 (trans 'N'), C is 6 x 6"),
    ("herk", "trans = b'C'", K1 + "A is 6 x 4 (trans 'C'), C is 6 x 6"),
    ("her2k", "db.n = 3", (K2, "and B (6 x 3, block 2 x 2, source 0,0) differ")),
    ("her2k", "db.mb = db.nb = 3", (K2, "and B (6 x 4, block 3 x 3, source 0,0) differ")),
    ("her2k", "db.jsrc = 1", (K2, "and B (6 x 4, block 2 x 2, source 0,1) differ")),
    ("herk", "da.mb = 3", K1 + "the operands need one square block (A 3 x 2, C 2 x 2)"),
    ("herk", "dc.mb = dc.nb = 3", K1 + "the operands need one square block (A 2 x 2, C 3 x 3)"),
    ("herk", "da.jsrc = 1", K1 + "source rank (0,1) outside the 1 x 1 grid"),
    ("herk", "dc.i = 1", K1 + "sub-matrices are not supported"),
    ("her2k", "db.j = 2", K2 + "sub-matrices are not supported"),
    ("pdsyrk", "ic = 2", (K1, "ia, ja, ic, jc must be 1")),
    ("pdsyr2k", "jb = 2", (K2, "ia, ja, ib, jb, ic, jc must be 1")),
    ("pdsyrk", "sc[0] = 2", (K1, "(dtype) must be 1")),
    ("pdsyrk", "sa[1] = ctx - 1", (K1, "A and C live on different contexts")),
    ("pdsyr2k", "sb[1] = ctx - 1", (K2, "A, B and C live on different contexts")),
    ("pdsyrk", "uplo = b'Q'", K1 + "bad uplo/trans 'Q' 'N'"),
])
def test_rank_update_preconditions_terminate(entry, mutate, needle):
    _terminates(SINGLE, entry, mutate, needle)


@pytest.mark.parametrize("entry,mutate,needle", [
    ("herk", "da.isrc = 1", K1 + "A must start on C's process row (source row 1 vs 0)"),
    ("her2k", "da.isrc = db.isrc = 1", K2 + "A must start on C's process row (source row 1 vs 0)"),
    ("herk", "dc.isrc = 2", K1 + "source rank (2,0) outside the 2 x 2 grid"),
    ("herk", "trans = b'C'; da.m, da.n = 4, 6", K1 + "trans 'C' on a 2 x 2 grid: only 'N' is built on more than one process"),
    ("her2k", "trans = b'T'; da.m, da.n = 4, 6; db.m, db.n = 4, 6", K2 + "trans 'T' on a 2 x 2 grid"),
    ("pdsyrk", "trans = b'T'", K1 + "trans 'T' on a 2 x 2 grid"),
])
def test_rank_update_grid_preconditions_terminate(entry, mutate, needle):
    """On a 2 x 2 host grid (no broadcast is ever made) the alignment rule and the refusal of trans C / T fire."""
    _terminates(HOST_2X2, entry, mutate, needle)


def test_rank_update_empty_and_quick_return_without_a_gpu():
    """n = 0 returns, and so does alpha = 0 / k = 0 with beta = 1, before the GPU is touched; C keeps its bits"""
    r = _run(PRELUDE + SINGLE + DESCS + "da.m = dc.m = dc.n = 0\n" + CALLS["herk"] + "\nr1 = r\n"
             "da.m = dc.m = dc.n = 6; be[0] = 1.0; al[0] = 0.0; c[:] = np.nan; a[:] = np.nan\n" + CALLS["herk"] + "\nr2 = r\n"
             "al[0] = 1.0; da.n = db.n = 0\n" + CALLS["her2k"] + "\nprint('codes', r1, r2, r, int(np.isnan(c).all()))")
    assert r.returncode == 0 and r.stdout.split() == ["codes", "0", "0", "0", "1"], (r.stdout, r.stderr[-800:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]
