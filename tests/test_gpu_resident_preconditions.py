"""The refusals of the resident triangular solver, triangular multiplication and Hermitian multiplication
(dlaf_mi355x_*_device): they are judged by the functions that judge the descriptor entries (require_triangular,
require_hermitian_multiplication in csrc/host/api_checks.hpp) and print the same sentences, plus the one a host array
cannot provoke -- the triangle a resident matrix holds.  A handle cannot be made without a device, so these are GPU
tests; each makes two or three handles of order 6 with block 2 and expects the process to end with the routine's
message before any sweep is launched.  The source-process cases run on a 2 x 2 host grid on which no broadcast is ever
made (this process is rank 0 of it)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = "g = d.Grid.single()"
HOST_2X2 = "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)"

A_L = "A = d.DeviceMatrix(g, np.float64, 'L', 6, 2)"
B_64 = "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2)"
C_64 = "Cm = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2)"

TRI = {"solver": "triangular solver", "multiplication": "triangular multiplication"}
TRI_CASES = [
    (SINGLE, "A = d.DeviceMatrix(g, np.float64, 'U', 6, 2)", B_64, "L",
     "{who}: uplo 'L' but the resident matrix holds its 'U' triangle\n"),
    (SINGLE, A_L, B_64, "R", "{who}: A is 6 x 6, B is 6 x 4 (side R)\n"),
    (SINGLE, A_L, "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 3)", "L",
     "{who}: B's blocks (3 x 3) do not match A's (2 x 2) for side L\n"),
    (HOST_2X2, A_L, "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2, isrc=1)", "L",
     "{who}: A and B must share the source process along the triangular dimension\n"),
]
HEMM = "[dlaf_mi355x] hermitian multiplication: "
HEMM_CASES = [
    (SINGLE, "A = d.DeviceMatrix(g, np.float64, 'U', 6, 2)", B_64, C_64, "L",
     HEMM + "uplo 'L' but the resident matrix holds its 'U' triangle\n"),
    (SINGLE, A_L, B_64, C_64, "R", HEMM + "A is 6 x 6, B and C are 6 x 4 (side R)\n"),
    (SINGLE, A_L, B_64, "Cm = d.GeneralDeviceMatrix(g, np.float64, 6, 5, 2)", "L",
     HEMM + "B (6 x 4, blocks 2 x 2) and C (6 x 5, blocks 2 x 2) differ\n"),
    (SINGLE, A_L, "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 3)", "Cm = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 3)",
     "L", HEMM + "the blocks of B and C (3 x 3) do not match A's (2 x 2) for side L\n"),
    (HOST_2X2, A_L, "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2, jsrc=1)", C_64, "L",
     HEMM + "B and C must share the source process ((0,1) vs (0,0))\n"),
    (HOST_2X2, A_L, "B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2, isrc=1)",
     "Cm = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2, isrc=1)", "L",
     HEMM + "A must share the source process of B and C along A's dimension\n"),
]


def _refused(lines, needle):
    code = "\n".join(["import numpy as np, dla_future_amd as d", "d.initialize()"] + lines + ["print('survived')"]) + "\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    assert needle in r.stderr, (needle, r.stderr[-800:])


@pytest.mark.parametrize("grid,a,b,side,needle", TRI_CASES)
@pytest.mark.parametrize("routine", sorted(TRI))
def test_resident_triangular_refusals(routine, grid, a, b, side, needle):
    _refused([grid, a, b, f"d.triangular_{routine}_device('{side}', 'L', 'N', 'N', 1.0, A, B)"],
             needle.format(who="[dlaf_mi355x] " + TRI[routine]))


@pytest.mark.parametrize("grid,a,b,c,side,needle", HEMM_CASES)
def test_resident_hermitian_multiplication_refusals(grid, a, b, c, side, needle):
    _refused([grid, a, b, c, f"d.hermitian_multiplication_device('{side}', 'L', 1.0, A, B, 0.0, Cm)"], needle)
