"""CPU tests of the host side of triangular_inverse / inverse_from_cholesky_factor (no GPU): the entries are exported,
the index arithmetic of the two sweeps (dlaf_mi355x_inverse_plan / _step: the progression of the local diagonal tiles
that one batched launch covers, the local ranges of "row k left of the diagonal" and "the rows below k", the owners
that root the broadcasts, the workspace size) agrees with a brute-force enumeration over every rank of the grids and
geometries the multiplication's host-logic tests use, and bad arguments terminate before the GPU is touched."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = [f"dlaf_mi355x_{name}_{t}" for name in ("triangular_inverse", "inverse_from_cholesky_factor") for t in "sdcz"] + \
          [f"dlaf_mi355x_p{t}{name}" for name in ("trtri", "potri") for t in "sdcz"] + \
          ["dlaf_mi355x_triangular_inverse_device", "dlaf_mi355x_inverse_from_cholesky_factor_device",
           "dlaf_mi355x_inverse_profile", "dlaf_mi355x_inverse_plan", "dlaf_mi355x_inverse_step"]
GRIDS = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 2), (4, 6)]
SHAPES = [(0, 4), (1, 4), (6, 2), (19, 6), (25, 5), (70, 8), (333, 100), (400, 64)]


def test_inverse_entries_exported():
    import dla_future_amd as d
    from dla_future_amd.capi import SIGNATURES
    L = C.CDLL(d.lib_path())
    for name in ENTRIES:
        assert hasattr(L, name) and name in SIGNATURES, name
    for name in ("triangular_inverse", "inverse_from_cholesky_factor", "pxtrtri", "pxpotri", "inverse_profile"):
        assert callable(getattr(d, name)) and name in d.__all__, name
    assert callable(d.DeviceMatrix.invert_triangular) and callable(d.DeviceMatrix.invert_from_factor)


@pytest.mark.parametrize("pr,pc", GRIDS)
def test_plan_and_steps_against_enumeration(pr, pc):
    from dla_future_amd.capi import lib
    for (n, nb), (sr, sc) in itertools.product(SHAPES, [(0, 0), (pr - 1, min(2, pc - 1))]):
        nt = -(-n // nb)
        for r, c in itertools.product(range(pr), range(pc)):
            rows = [k for k in range(nt) if (k + sr) % pr == r]   # global tiles of my local tile rows, in local order
            cols = [k for k in range(nt) if (k + sc) % pc == c]
            diag = [k for k in rows if k in cols]
            plan = (C.c_long * 9)()
            assert lib().dlaf_mi355x_inverse_plan(n, nb, pr, pc, r, c, sr, sc, plan) == 0
            count, k0, kstep, il0, jl0, ils, jls, last, ws = list(plan)
            assert count == len(diag), (n, nb, r, c)
            # one arithmetic progression in k, in the local row and in the local column
            assert [k0 + m * kstep for m in range(count)] == diag
            assert [il0 + m * ils for m in range(count)] == [rows.index(k) for k in diag]
            assert [jl0 + m * jls for m in range(count)] == [cols.index(k) for k in diag]
            if count:
                assert last == min(nb, n - diag[-1] * nb)
            # panels, never n^2: the row panel, the column panel, two tiles per local diagonal tile and a received pair
            assert ws == len(rows) + len(cols) + 2 * (count + 1)
            for k in range(nt):
                st = (C.c_long * 7)()
                assert lib().dlaf_mi355x_inverse_step(n, nb, pr, pc, r, c, sr, sc, k, st) == 0
                own_r, own_c, il_below, nrl, ncl, lr, lc = list(st)
                assert (own_r, own_c) == ((k + sr) % pr, (k + sc) % pc)
                assert il_below == sum(1 for g in rows if g <= k) and rows[il_below:] == [g for g in rows if g > k]
                assert rows[:nrl] == [g for g in rows if g < k] and cols[:ncl] == [g for g in cols if g < k]
                assert lr == (rows.index(k) if k in rows else -1) and lc == (cols.index(k) if k in cols else -1)


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "a = np.eye(6, order='F'); da = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
           "uplo, diag = 'L', 'N'\n")


@pytest.mark.parametrize("mutate,needle", [
    ("uplo = 'Q'", "uplo must be 'L' or 'U'"),
    ("da.isrc = 3", "outside the 1 x 1 grid"),
    ("da.jsrc = 1", "outside the 1 x 1 grid"),
])
def test_inverse_preconditions_terminate(mutate, needle):
    r = _run(PRELUDE + "g = d.Grid.single()\n" + f"{mutate}\n"
             "lib().dlaf_mi355x_triangular_inverse_d(g.context, uplo.encode(), diag.encode(), a.ctypes.data, da)\n"
             "print('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and needle in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


def test_pxtrtri_bad_offsets_terminate():
    r = _run("import numpy as np, dla_future_amd as d\n"
             "g = d.Grid.single(); a = np.eye(4, order='F')\n"
             "d.pxpotri('L', 4, a, 2, 1, [1, g.context, 4, 4, 2, 2, 0, 0, 4])\n"
             "print('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and "ia, ja must be 1" in r.stderr, r.stderr[-500:]
