"""The triangular solver on the grid (dlaf_mi355x_triangular_solver_*, dlaf_mi355x_p?trsm; csrc/host/solver.cpp)."""
from __future__ import annotations

import numpy as np

from . import _triangular
from ._abi import two_doubles
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def triangular_solver(grid: Grid, side: str, uplo: str, op: str, diag: str, alpha, a: np.ndarray, b: np.ndarray,
                      nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), b_src=(0, 0),
                      b_block: tuple[int, int] | None = None) -> None:
    """dlaf::triangular_solver(grid, side, uplo, op, diag, alpha, A, B)
    (include/dlaf/solver/triangular.h:41-177) == dlaf_mi355x_triangular_solver_{s,d,c,z}:
    side 'L': op(A) X = alpha B, side 'R': X op(A) = alpha B; `b` (this process's local column-major part of
    the m x n right-hand sides) is overwritten by X.  `a`: local part of the triangular matrix.
    `nb`: the square block of A; `b_block` = (MB, NB) of B when they differ (triangular.h:41-60: B's block along the
    triangular dimension must be A's, the other one is free)."""
    _triangular.on_grid("solver", grid, side, uplo, op, diag, alpha, a, b, nb, m, n, a_src, b_src, b_block)


def pxtrsm(side: str, uplo: str, op: str, diag: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}trsm: ScaLAPACK's p?trsm argument list (9-int descriptors)."""
    _triangular.scalapack("trsm", side, uplo, op, diag, m, n, alpha, a, ia, ja, desca, b, ib, jb, descb)


def triangular_solver_device(side: str, uplo: str, op: str, diag: str, alpha, a: DeviceMatrix, b: GeneralDeviceMatrix) -> None:
    """dlaf::triangular_solver on resident operands: `a` holds the triangular matrix in its uplo triangle (e.g. the
    factor a.factorize() left there), `b` is overwritten by the solution; no PCIe traffic."""
    _triangular.resident("solver", side, uplo, op, diag, alpha, a, b)


def solver_profile():
    """(ms, flops) of the sweep of the last triangular solve on this process (device time, no staging)."""
    return two_doubles("dlaf_mi355x_solver_profile")
