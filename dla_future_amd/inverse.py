"""The inverse of a triangular matrix and of a matrix from its Cholesky factor (dlaf_mi355x_triangular_inverse_*,
dlaf_mi355x_inverse_from_cholesky_factor_*, dlaf_mi355x_p?trtri, p?potri; csrc/host/inverse.cpp).  The resident forms are
methods of DeviceMatrix."""
from __future__ import annotations

import numpy as np

from ._abi import desc9, entry, global_size, info_of, ld_of, make_descriptor, ptr, two_doubles
from .capi import type_char
from .grid import Grid


def triangular_inverse(grid: Grid, uplo: str, diag: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                       n: int | None = None) -> int:
    """dlaf::triangular_inverse == dlaf_mi355x_triangular_inverse_{s,d,c,z} (LAPACK xTRTRI): the triangular matrix in the
    uplo triangle of `a` (this process's local part; diag 'N' / 'U') is overwritten by its inverse.  Returns LAPACK's
    info: i > 0 when the i-th diagonal element is exactly zero, and `a` is then untouched."""
    t = type_char(a.dtype)
    da = make_descriptor(global_size(grid, n, a), nb, ld_of(a), isrc, jsrc)
    return entry(f"dlaf_mi355x_triangular_inverse_{t}")(grid.context, uplo.encode(), diag.encode(), ptr(a), da)


def inverse_from_cholesky_factor(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                                 n: int | None = None) -> int:
    """dlaf::inverse_from_cholesky_factor == dlaf_mi355x_inverse_from_cholesky_factor_{s,d,c,z} (LAPACK xPOTRI): the
    uplo triangle of `a` holds the Cholesky factor and is overwritten by the same triangle of inv(L L^H) / inv(U^H U).
    Returns LAPACK's info."""
    t = type_char(a.dtype)
    da = make_descriptor(global_size(grid, n, a), nb, ld_of(a), isrc, jsrc)
    return entry(f"dlaf_mi355x_inverse_from_cholesky_factor_{t}")(grid.context, uplo.encode(), ptr(a), da)


def pxtrtri(uplo: str, diag: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_mi355x_p{s,d,c,z}trtri: ScaLAPACK's p?trtri argument list; returns info."""
    return info_of(f"dlaf_mi355x_p{type_char(a.dtype)}trtri", uplo.encode(), diag.encode(), n, ptr(a), ia, ja, desc9(desca))


def pxpotri(uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_mi355x_p{s,d,c,z}potri: ScaLAPACK's p?potri argument list; returns info."""
    return info_of(f"dlaf_mi355x_p{type_char(a.dtype)}potri", uplo.encode(), n, ptr(a), ia, ja, desc9(desca))


def inverse_profile():
    """(ms, flops) of the last triangular_inverse / inverse_from_cholesky_factor on this process (device time, no
    staging; n^3 / 3 flops per half, x 4 for complex types)."""
    return two_doubles("dlaf_mi355x_inverse_profile")
