"""The generalized Hermitian eigenproblem brought to standard form (dlaf_mi355x_generalized_to_standard_*,
dlaf_mi355x_p?hegst; csrc/host/gen_to_std.cpp).  The resident form is a method of DeviceMatrix."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import desc9, entry, global_size, ld_of, make_descriptor, ptr
from .capi import type_char
from .grid import Grid


def generalized_to_standard(grid: Grid, uplo: str, a: np.ndarray, b: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                            n: int | None = None) -> int:
    """dlaf::eigensolver::internal::generalized_to_standard(grid, uplo, mat_a, mat_b)
    (include/dlaf/eigensolver/gen_to_std.h:50, :101) == dlaf_mi355x_generalized_to_standard_{s,d,c,z}:
    `a` (this process's local part of the Hermitian A) is overwritten by inv(L) A inv(L^H) (uplo 'L') or
    inv(U^H) A inv(U) (uplo 'U') in its uplo triangle; `b` holds the Cholesky factor of B in the same triangle."""
    t = type_char(a.dtype)
    if a.dtype != b.dtype:
        raise ValueError("A and B must have the same element type")
    n = global_size(grid, n, a)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    db = make_descriptor(n, nb, ld_of(b), isrc, jsrc)
    return entry(f"dlaf_mi355x_generalized_to_standard_{t}")(grid.context, uplo.encode(), ptr(a), da, ptr(b), db)


def pxhegst(ibtype: int, uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb):
    """dlaf_mi355x_p{s,d,c,z}hegst: ScaLAPACK's p?sygst / p?hegst argument list; returns (scale, info)."""
    t = type_char(a.dtype)
    scale = (C.c_float if t in "sc" else C.c_double)(-1)
    info = C.c_int(-999)
    entry(f"dlaf_mi355x_p{t}hegst")(ibtype, uplo.encode(), n, ptr(a), ia, ja, desc9(desca), ptr(b), ib, jb, desc9(descb),
                                    C.byref(scale), C.byref(info))
    return scale.value, info.value
