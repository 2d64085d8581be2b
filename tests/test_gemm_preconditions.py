"""CPU tests of the general multiplication's preconditions (csrc/host/api_checks.hpp: require_general_multiplication,
behind the descriptor entries, p?gemm and the resident entry), in the style of test_c_api_preconditions.py: each case
changes one argument of an otherwise valid 6 x 6 x 6 call with block 2 and expects the routine's message on stderr
before the GPU is touched (the subprocesses run with the GPU hidden)."""
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
           "a = np.eye(6, order='F'); b = np.eye(6, order='F'); c = np.zeros((6, 6), order='F')\n"
           "al = np.array([1.0]); be = np.array([0.0])\n"
           "da, db, dc = (DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6) for _ in range(3))\n"
           "opa = opb = b'N'; ia = ja = ib = jb = ic = jc = 1; m = n = k = 6\n")
DESCS = ("ctx = g.context\n"
         "sa, sb, sc = ((C.c_int * 9)(1, ctx, 6, 6, 2, 2, 0, 0, 6) for _ in range(3))\n")
CALLS = {
    "gemm": "r = L.dlaf_mi355x_general_multiplication_d(ctx, opa, opb, al.ctypes.data, a.ctypes.data, da, b.ctypes.data, db, "
            "be.ctypes.data, c.ctypes.data, dc)",
    "pdgemm": "r = L.dlaf_mi355x_pdgemm(opa, opb, m, n, k, al.ctypes.data, a.ctypes.data, ia, ja, sa, b.ctypes.data, ib, jb, "
              "sb, be.ctypes.data, c.ctypes.data, ic, jc, sc)",
}
WHO = "general multiplication: "


def _terminates(grid, entry, mutate, needle):
    r = _run(PRELUDE + grid + DESCS + f"{mutate}\n" + CALLS[entry] + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    for part in ((needle,) if isinstance(needle, str) else needle):
        assert part in r.stderr, (part, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("entry,mutate,needle", [
    ("gemm", "opa = b'Q'", WHO + "bad opa/opb 'Q' 'N'"),
    ("gemm", "opb = b'x'", WHO + "bad opa/opb 'N' 'x'"),
    ("gemm", "da.n = 5", WHO + "op(A) is 6 x 5 (op 'N'), op(B) is 6 x 6 (op 'N'), C is 6 x 6"),
    ("gemm", "da.m = 5; opa = b'T'", WHO + "op(A) is 6 x 5 (op 'T')"),
    ("gemm", "db.n = 4", (WHO, "op(B) is 6 x 4 (op 'N'), C is 6 x 6")),
    ("gemm", "db.mb = db.nb = 3", WHO + "A, B and C need one square block (A 2 x 2, B 3 x 3, C 2 x 2)"),
    ("gemm", "dc.mb = 3", WHO + "A, B and C need one square block (A 2 x 2, B 2 x 2, C 3 x 2)"),
    ("gemm", "da.jsrc = 1", WHO + "source rank (0,1) outside the 1 x 1 grid"),
    ("gemm", "dc.i = 1", WHO + "sub-matrices are not supported"),
    ("pdgemm", "ib = 2", (WHO, "ia, ja, ib, jb, ic, jc must be 1")),
    ("pdgemm", "sc[0] = 2", (WHO, "(dtype) must be 1")),
    ("pdgemm", "sb[1] = ctx - 1", (WHO, "A, B and C live on different contexts")),
    ("pdgemm", "opa = b'Q'", WHO + "bad opa/opb 'Q' 'N'"),
])
def test_general_multiplication_preconditions_terminate(entry, mutate, needle):
    _terminates(SINGLE, entry, mutate, needle)


@pytest.mark.parametrize("entry,mutate,needle", [
    ("gemm", "da.isrc = 1", WHO + "A must start on C's process row (source row 1 vs 0)"),
    ("gemm", "db.jsrc = 1", WHO + "B must start on C's process column (source column 1 vs 0)"),
    ("gemm", "dc.isrc = 2", WHO + "source rank (2,0) outside the 2 x 2 grid"),
    ("gemm", "opa = b'T'", WHO + "opa 'T', opb 'N' on a 2 x 2 grid: only 'N' 'N' is built on more than one process"),
    ("gemm", "opb = b'C'", WHO + "opa 'N', opb 'C' on a 2 x 2 grid: only 'N' 'N' is built on more than one process"),
    ("pdgemm", "opb = b'T'", WHO + "opa 'N', opb 'T' on a 2 x 2 grid"),
])
def test_general_multiplication_grid_preconditions_terminate(entry, mutate, needle):
    """On a 2 x 2 host grid (no broadcast is ever made) the alignment rule and the refusal of transposed ops fire."""
    _terminates(HOST_2X2, entry, mutate, needle)


def test_general_multiplication_empty_returns_without_a_gpu():
    r = _run(PRELUDE + SINGLE + DESCS + "da.m = dc.m = 0\n" + CALLS["gemm"] + "\nr1 = r\ndc.m = da.m = 6; db.n = dc.n = 0\n" +
             CALLS["gemm"] + "\nprint('codes', r1, r)")
    assert r.returncode == 0 and r.stdout.split() == ["codes", "0", "0"], (r.stdout, r.stderr[-800:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]
