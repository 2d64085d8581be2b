"""Addition, transposition, copy and Hermitian completion on the grid (dlaf_mi355x_general_addition_*,
dlaf_mi355x_hermitian_complete_*, dlaf_mi355x_p?geadd, p?tradd, p?tran / p?tranu / p?tranc, p?lacpy; csrc/host/addition.cpp)."""
from __future__ import annotations

import numpy as np

from ._abi import check, desc9, descriptor, entry, global_size, global_sizes, ld_of, ptr, scalar, two_doubles
from .capi import type_char
from .device_matrix import GeneralDeviceMatrix
from .grid import Grid


def general_addition(grid: Grid, uplo: str, op: str, alpha, a: np.ndarray, beta, c: np.ndarray, nb: int,
                     m: int | None = None, n: int | None = None, a_src=(0, 0), c_src=(0, 0)) -> None:
    """C = beta C + alpha op(A) on the uplo part of the m x n matrix C == dlaf_mi355x_general_addition_{s,d,c,z} (PBLAS
    p?geadd / p?tradd, p?tran / p?tranu / p?tranc; ScaLAPACK p?lacpy is alpha 1, beta 0, op 'N').  uplo 'A' all, 'L' i >= j,
    'U' i <= j; op 'N' (A stored m x n), 'T' or 'C' (A stored n x m).  `a`, `c`: this process's local column-major parts;
    outside the uplo part `c` stays bit for bit; alpha 1, beta 0 with op 'N' / 'T' is a bit copy.  nb: the square block of
    both.  Any grid (m and n are required on more than one process); op 'N' needs A on C's source process, and only op
    'N' accepts `a is c`."""
    t = type_char(c.dtype)
    if a.dtype != c.dtype:
        raise ValueError("A and C must have the same element type")
    m, n = global_sizes(grid, (m, n), c.shape, "the global sizes m, n are")
    tn = op.upper() == "N"
    da = descriptor(m if tn else n, n if tn else m, nb, a_src, ld_of(a))
    dc = descriptor(m, n, nb, c_src, ld_of(c))
    check(f"dlaf_mi355x_general_addition_{t}", grid.context, uplo.encode(), op.encode(), scalar(alpha, c.dtype), ptr(a), da,
          scalar(beta, c.dtype), ptr(c), dc)


def hermitian_complete(grid: Grid, uplo: str, kind: str, a: np.ndarray, nb: int, n: int | None = None, src=(0, 0)) -> None:
    """Fills the OTHER triangle of the n x n matrix from its uplo one, in place == dlaf_mi355x_hermitian_complete_{s,d,c,z}:
    kind 'H' conjugates the mirror and makes the diagonal's imaginary parts exactly 0, kind 'S' transposes plainly and
    leaves the diagonal untouched.  `a`: this process's local column-major part; nb: its square block."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    check(f"dlaf_mi355x_hermitian_complete_{t}", grid.context, uplo.encode(), kind.encode(), ptr(a),
          descriptor(n, n, nb, src, ld_of(a)))


def _scalapack(routine: str, letters, m, n, alpha, a, ia, ja, desca, beta, c, ic, jc, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}<routine>: `letters` in front of PBLAS's (m, n, alpha, A, beta, C) argument list."""
    entry(f"dlaf_mi355x_p{type_char(c.dtype)}{routine}")(
        *(x.encode() for x in letters), m, n, scalar(alpha, c.dtype), ptr(a), ia, ja, desc9(desca), scalar(beta, c.dtype),
        ptr(c), ic, jc, desc9(descc))


def pxgeadd(trans: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray, ic: int,
            jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}geadd: PBLAS's argument list (9-int descriptors): C = beta C + alpha op(A)."""
    _scalapack("geadd", (trans,), m, n, alpha, a, ia, ja, desca, beta, c, ic, jc, descc)


def pxtradd(uplo: str, trans: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray,
            ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}tradd: the same on the uplo ('L' / 'U') trapezoid of C."""
    _scalapack("tradd", (uplo, trans), m, n, alpha, a, ia, ja, desca, beta, c, ic, jc, descc)


def pxtran(m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray, ic: int, jc: int, descc,
           conj: bool = False) -> None:
    """dlaf_mi355x_p{s,d}tran / p{c,z}tranu (conj False) / p{c,z}tranc (conj True): C (m x n) = beta C + alpha A^T / A^H,
    A stored n x m."""
    suffix = ("c" if conj else "u") if type_char(c.dtype) in "cz" else ""
    _scalapack("tran" + suffix, (), m, n, alpha, a, ia, ja, desca, beta, c, ic, jc, descc)


def pxlacpy(uplo: str, m: int, n: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}lacpy: B = A on the uplo part; as in LAPACK any letter other than 'U' / 'L' means all."""
    entry(f"dlaf_mi355x_p{type_char(b.dtype)}lacpy")(uplo.encode(), m, n, ptr(a), ia, ja, desc9(desca), ptr(b), ib, jb,
                                                    desc9(descb))


def general_addition_device(uplo: str, op: str, alpha, a: GeneralDeviceMatrix, beta, c: GeneralDeviceMatrix) -> None:
    """general_addition on resident general matrices (`a` as stored; only the uplo part of `c` is written; `a is c` is op
    'N' in place); no PCIe traffic."""
    check("dlaf_mi355x_general_addition_device", uplo.encode(), op.encode(), scalar(alpha, c.dtype), a._h,
          scalar(beta, c.dtype), c._h)


def hermitian_complete_device(uplo: str, kind: str, a: GeneralDeviceMatrix) -> None:
    """hermitian_complete on a resident general matrix, in place; no PCIe traffic."""
    check("dlaf_mi355x_hermitian_complete_device", uplo.encode(), kind.encode(), a._h)


def addition_profile():
    """(ms, bytes) of the last general_addition / hermitian_complete / conversion on this process: device time, and the
    whole-grid algorithmic bytes (read A + write C, + read C when beta != 0; a completion reads and writes half)."""
    return two_doubles("dlaf_mi355x_addition_profile")
