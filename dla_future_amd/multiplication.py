"""Triangular, Hermitian and general multiplication on the grid (dlaf_mi355x_{triangular,hermitian,general}_multiplication_*,
dlaf_mi355x_p?trmm, p?symm / p?hemm, p?gemm; csrc/host/multiplication.cpp)."""
from __future__ import annotations

import numpy as np

from . import _triangular
from ._abi import check, desc9, descriptor, entry, global_sizes, ld_of, ptr, scalar, two_doubles
from .capi import type_char
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def triangular_multiplication(grid: Grid, side: str, uplo: str, op: str, diag: str, alpha, a: np.ndarray, b: np.ndarray,
                              nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), b_src=(0, 0),
                              b_block: tuple[int, int] | None = None) -> None:
    """dlaf::triangular_multiplication(grid, side, uplo, op, diag, alpha, A, B)
    (include/dlaf/multiplication/triangular.h) == dlaf_mi355x_triangular_multiplication_{s,d,c,z}:
    side 'L': B = alpha op(A) B, side 'R': B = alpha B op(A); `b` (this process's local column-major part of the
    m x n matrix B) is overwritten.  The other arguments are triangular_solver's."""
    _triangular.on_grid("multiplication", grid, side, uplo, op, diag, alpha, a, b, nb, m, n, a_src, b_src, b_block)


def pxtrmm(side: str, uplo: str, op: str, diag: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}trmm: ScaLAPACK's p?trmm argument list (9-int descriptors)."""
    _triangular.scalapack("trmm", side, uplo, op, diag, m, n, alpha, a, ia, ja, desca, b, ib, jb, descb)


def triangular_multiplication_device(side: str, uplo: str, op: str, diag: str, alpha, a: DeviceMatrix,
                                     b: GeneralDeviceMatrix) -> None:
    """dlaf::triangular_multiplication on resident operands: `a` holds the triangular matrix in its uplo triangle
    (e.g. the factor a.factorize() left there), `b` is overwritten by the product; no PCIe traffic."""
    _triangular.resident("multiplication", side, uplo, op, diag, alpha, a, b)


def _same_type(a, b, c) -> str:
    t = type_char(c.dtype)
    if a.dtype != c.dtype or b.dtype != c.dtype:
        raise ValueError("A, B and C must have the same element type")
    return t


def hermitian_multiplication(grid: Grid, side: str, uplo: str, alpha, a: np.ndarray, b: np.ndarray, beta, c: np.ndarray,
                             nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), c_src=(0, 0),
                             c_block: tuple[int, int] | None = None) -> None:
    """dlaf::hermitian_multiplication(grid, side, uplo, alpha, A, B, beta, C) (include/dlaf/multiplication/hermitian.h)
    == dlaf_mi355x_hermitian_multiplication_{s,d,c,z}: side 'L': C = beta C + alpha A B, side 'R': C = beta C + alpha B A
    with A Hermitian (only its uplo triangle is read).  `a`, `b`, `c`: this process's local column-major parts; `c` is
    overwritten.  nb: A's square block; c_block: the MB x NB blocks of B and C (their block along A's dimension must be
    nb); c_src: the source process of B and C."""
    t = _same_type(a, b, c)
    m, n = global_sizes(grid, (m, n), c.shape, "the global size m x n of C is")
    na = m if side.upper() == "L" else n
    da = descriptor(na, na, nb, a_src, ld_of(a))
    block = c_block if c_block is not None else nb
    db = descriptor(m, n, block, c_src, ld_of(b))
    dc = descriptor(m, n, block, c_src, ld_of(c))
    check(f"dlaf_mi355x_hermitian_multiplication_{t}", grid.context, side.encode(), uplo.encode(), scalar(alpha, c.dtype),
          ptr(a), da, ptr(b), db, scalar(beta, c.dtype), ptr(c), dc)


def pxhemm(side: str, uplo: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int,
           jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d}symm / p{c,z}hemm: ScaLAPACK's argument list (9-int descriptors)."""
    t = type_char(c.dtype)
    entry(f"dlaf_mi355x_p{t}{'hemm' if t in 'cz' else 'symm'}")(
        side.encode(), uplo.encode(), m, n, scalar(alpha, c.dtype), ptr(a), ia, ja, desc9(desca), ptr(b), ib, jb,
        desc9(descb), scalar(beta, c.dtype), ptr(c), ic, jc, desc9(descc))


def general_multiplication(grid: Grid, opa: str, opb: str, alpha, a: np.ndarray, b: np.ndarray, beta, c: np.ndarray,
                           nb: int, m: int | None = None, n: int | None = None, k: int | None = None, a_src=(0, 0),
                           b_src=(0, 0), c_src=(0, 0)) -> None:
    """dlaf::multiplication::internal::generalMatrix(opA, opB, alpha, A, B, beta, C) (include/dlaf/multiplication/general.h)
    == dlaf_mi355x_general_multiplication_{s,d,c,z}: C = beta C + alpha op(A) op(B), op 'N', 'T' or 'C'.  `a`, `b`, `c`:
    this process's local column-major parts of the matrices as stored (A is m x k for 'N', k x m otherwise; B is k x n
    for 'N', n x k otherwise); `c` is overwritten.  nb: the square block of all three.  On a grid of more than one
    process only 'N' 'N' is built, m, n, k are required, A must start on C's process row and B on C's process column."""
    t = _same_type(a, b, c)
    an, bn = opa.upper() == "N", opb.upper() == "N"
    m, n, k = global_sizes(grid, (m, n, k), lambda: (*c.shape, a.shape[1] if an else a.shape[0]),
                           "the global sizes m, n, k are")
    da = descriptor(m if an else k, k if an else m, nb, a_src, ld_of(a))
    db = descriptor(k if bn else n, n if bn else k, nb, b_src, ld_of(b))
    dc = descriptor(m, n, nb, c_src, ld_of(c))
    check(f"dlaf_mi355x_general_multiplication_{t}", grid.context, opa.encode(), opb.encode(), scalar(alpha, c.dtype), ptr(a),
          da, ptr(b), db, scalar(beta, c.dtype), ptr(c), dc)


def pxgemm(transa: str, transb: str, m: int, n: int, k: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}gemm: ScaLAPACK's argument list (9-int descriptors)."""
    entry(f"dlaf_mi355x_p{type_char(c.dtype)}gemm")(
        transa.encode(), transb.encode(), m, n, k, scalar(alpha, c.dtype), ptr(a), ia, ja, desc9(desca), ptr(b), ib, jb,
        desc9(descb), scalar(beta, c.dtype), ptr(c), ic, jc, desc9(descc))


def _resident(kind: str, x: str, y: str, alpha, a, b, beta, c) -> None:
    """kind: "hermitian" (x, y = side, uplo) or "general" (x, y = opa, opb)."""
    check(f"dlaf_mi355x_{kind}_multiplication_device", x.encode(), y.encode(), scalar(alpha, c.dtype), a._h, b._h,
          scalar(beta, c.dtype), c._h)


def hermitian_multiplication_device(side: str, uplo: str, alpha, a: DeviceMatrix, b: GeneralDeviceMatrix, beta,
                                    c: GeneralDeviceMatrix) -> None:
    """dlaf::hermitian_multiplication on resident operands: `a` holds the Hermitian matrix in its uplo triangle, `b` and
    `c` are general resident matrices of the same shape; only `c` is written; no PCIe traffic."""
    _resident("hermitian", side, uplo, alpha, a, b, beta, c)


def general_multiplication_device(opa: str, opb: str, alpha, a: GeneralDeviceMatrix, b: GeneralDeviceMatrix, beta,
                                  c: GeneralDeviceMatrix) -> None:
    """general_multiplication on resident operands: C = beta C + alpha op(A) op(B) on three general resident matrices
    (`a`, `b` as stored); only `c` is written; no PCIe traffic."""
    _resident("general", opa, opb, alpha, a, b, beta, c)


def multiplication_profile():
    """(ms, flops) of the sweep of the last multiplication (triangular, Hermitian, general or Hermitian rank update) on this
    process (device time, no staging)."""
    return two_doubles("dlaf_mi355x_multiplication_profile")
