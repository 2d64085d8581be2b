"""Host-side mirror of the reference's Cholesky interface over the C ABI.

Names and argument meaning follow the reference (file:line in the docstrings); arrays are numpy,
column-major ("F" order) like every DLA-Future local matrix.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import check, desc9, entry, global_size, info_of, ld_of, make_descriptor, ptr
from .capi import lib, type_char
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def cholesky_factorization(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                           n: int | None = None) -> int:
    """dlaf_cholesky_factorization_{s,d,c,z} (include/dlaf_c/factorization/cholesky.h:32-47) ==
    dlaf::cholesky_factorization(grid, uplo, matrix) (include/dlaf/factorization/cholesky.h:67-79).

    `a` is this process's local column-major part (host memory); factored in place in the `uplo`
    triangle.  Returns 0, or the LAPACK info of a non-positive-definite leading minor."""
    t = type_char(a.dtype)
    desc = make_descriptor(global_size(grid, n, a), nb, ld_of(a), isrc, jsrc)
    return entry(f"dlaf_cholesky_factorization_{t}")(grid.context, uplo.encode(), ptr(a), desc)


def pxpotrf(uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_p{s,d,c,z}potrf (include/dlaf_c/factorization/cholesky.h:74-87); desca is the 9-int
    ScaLAPACK descriptor {1, ctxt, M, N, MB, NB, RSRC, CSRC, LLD}.  Returns info."""
    return info_of(f"dlaf_p{type_char(a.dtype)}potrf", uplo.encode(), n, ptr(a), ia, ja, desc9(desca))


def pxpotrs(uplo: str, n: int, nrhs: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb) -> int:
    """dlaf_mi355x_p{s,d,c,z}potrs: A X = B with the factor p?potrf left in `a`; returns info."""
    return info_of(f"dlaf_mi355x_p{type_char(b.dtype)}potrs", uplo.encode(), n, nrhs, ptr(a), ia, ja, desc9(desca), ptr(b),
                   ib, jb, desc9(descb))


def potrs_device(uplo: str, factor: DeviceMatrix, b: GeneralDeviceMatrix) -> None:
    """A X = B from the resident Cholesky factor (the two solves of p?potrs, all in HBM)."""
    check("dlaf_mi355x_potrs_device", uplo.encode(), factor._h, b._h)


def set_random_hermitian_positive_definite(grid: Grid, a: np.ndarray, n: int, nb: int, isrc: int = 0,
                                           jsrc: int = 0, nthreads: int = 0) -> None:
    """matrix::util::set_random_hermitian_positive_definite (include/dlaf/util_matrix.h:498-501) on
    this process's local array."""
    desc = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    check("dlaf_mi355x_set_random_hpd", grid.context, type_char(a.dtype).encode(), ptr(a), desc, nthreads)


def potrf_trace():
    """Diagnosis hook (DLAF_MI355X_POTRF_TRACE=1): the 32 words the last first-diagonal-tile POTRF of this process
    recorded (kernels_potrf_coop.hip), or None when tracing is off."""
    out = (C.c_ulonglong * 32)()
    return list(out) if lib().dlaf_mi355x_potrf_trace(out) == 0 else None


def release_workspace_pool() -> int:
    """Give the idle blocks of the workspace pool back to the driver (dlaf_mi355x_workspace_pool_release); returns the bytes
    that were held."""
    return int(lib().dlaf_mi355x_workspace_pool_release())


def update_launch_stats():
    """(persistent, exclusive): trailing-update launches of this process so far in persistent form / with exclusive
    compute units."""
    a, b = C.c_long(0), C.c_long(0)
    lib().dlaf_mi355x_update_launch_stats(C.byref(a), C.byref(b))
    return a.value, b.value
