"""Hermitian rank-k and rank-2k updates on the grid (dlaf_mi355x_hermitian_rank_{k,2k}_update_*, dlaf_mi355x_p?syrk / p?herk,
p?syr2k / p?her2k; csrc/host/rank_update.cpp).  The weighted rank-k update is in matrix_function.py."""
from __future__ import annotations

import numpy as np

from ._abi import check, desc9, descriptor, entry, global_sizes, ld_of, ptr, real_dtype, scalar
from .capi import type_char
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def _rank_update(two: bool, grid: Grid, uplo: str, trans: str, alpha, a: np.ndarray, b, beta, c: np.ndarray, nb: int,
                 n, k, a_src, c_src) -> None:
    t = type_char(c.dtype)
    if a.dtype != c.dtype or (two and b.dtype != c.dtype):
        raise ValueError("the operands must have the same element type")
    tn = trans.upper() == "N"
    n, k = global_sizes(grid, (n, k), lambda: (c.shape[0], a.shape[1] if tn else a.shape[0]), "the global sizes n, k are")
    rdt = real_dtype(c.dtype)
    da = descriptor(n if tn else k, k if tn else n, nb, a_src, ld_of(a))
    dc = descriptor(n, n, nb, c_src, ld_of(c))
    if two:
        db = descriptor(n if tn else k, k if tn else n, nb, a_src, ld_of(b))
        check(f"dlaf_mi355x_hermitian_rank_2k_update_{t}", grid.context, uplo.encode(), trans.encode(), scalar(alpha, c.dtype),
              ptr(a), da, ptr(b), db, scalar(beta, rdt), ptr(c), dc)
    else:
        check(f"dlaf_mi355x_hermitian_rank_k_update_{t}", grid.context, uplo.encode(), trans.encode(), scalar(alpha, rdt),
              ptr(a), da, scalar(beta, rdt), ptr(c), dc)


def hermitian_rank_k_update(grid: Grid, uplo: str, trans: str, alpha, a: np.ndarray, beta, c: np.ndarray, nb: int,
                            n: int | None = None, k: int | None = None, a_src=(0, 0), c_src=(0, 0)) -> None:
    """xSYRK / xHERK on the grid == dlaf_mi355x_hermitian_rank_k_update_{s,d,c,z}: the uplo triangle of the n x n matrix C
    becomes alpha A A^H + beta C (trans 'N', A stored n x k) or alpha A^H A + beta C (trans 'C', A stored k x n); alpha
    and beta are real.  `a`, `c`: this process's local column-major parts; only the uplo triangle of `c` is read or
    written, and its diagonal comes back with imaginary part 0.  nb: the square block of both.  On a grid of more than
    one process only trans 'N' is built, n and k are required and A must start on C's process row."""
    _rank_update(False, grid, uplo, trans, alpha, a, None, beta, c, nb, n, k, a_src, c_src)


def hermitian_rank_2k_update(grid: Grid, uplo: str, trans: str, alpha, a: np.ndarray, b: np.ndarray, beta, c: np.ndarray,
                             nb: int, n: int | None = None, k: int | None = None, a_src=(0, 0), c_src=(0, 0)) -> None:
    """xSYR2K / xHER2K on the grid == dlaf_mi355x_hermitian_rank_2k_update_{s,d,c,z}: the uplo triangle of C becomes
    alpha A B^H + conj(alpha) B A^H + beta C (trans 'N') or alpha A^H B + conj(alpha) B^H A + beta C (trans 'C'); alpha
    is of the element type, beta is real; B is stored, blocked and distributed like A.  Otherwise as
    hermitian_rank_k_update."""
    _rank_update(True, grid, uplo, trans, alpha, a, b, beta, c, nb, n, k, a_src, c_src)


def pxherk(uplo: str, trans: str, n: int, k: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray,
           ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d}syrk / p{c,z}herk: ScaLAPACK's argument list (9-int descriptors; alpha and beta real)."""
    t, rdt = type_char(c.dtype), real_dtype(c.dtype)
    entry(f"dlaf_mi355x_p{t}{'herk' if t in 'cz' else 'syrk'}")(
        uplo.encode(), trans.encode(), n, k, scalar(alpha, rdt), ptr(a), ia, ja, desc9(desca), scalar(beta, rdt), ptr(c), ic,
        jc, desc9(descc))


def pxher2k(uplo: str, trans: str, n: int, k: int, alpha, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int,
            jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d}syr2k / p{c,z}her2k: ScaLAPACK's argument list (9-int descriptors; beta real)."""
    t = type_char(c.dtype)
    entry(f"dlaf_mi355x_p{t}{'her2k' if t in 'cz' else 'syr2k'}")(
        uplo.encode(), trans.encode(), n, k, scalar(alpha, c.dtype), ptr(a), ia, ja, desc9(desca), ptr(b), ib, jb,
        desc9(descb), scalar(beta, real_dtype(c.dtype)), ptr(c), ic, jc, desc9(descc))


def hermitian_rank_k_update_device(uplo: str, trans: str, alpha, a: GeneralDeviceMatrix, beta, c: DeviceMatrix) -> None:
    """hermitian_rank_k_update on resident operands: `c` a DeviceMatrix created with this uplo (what factorize() takes),
    `a` a general resident matrix as stored; only the uplo triangle of `c` is written; no PCIe traffic."""
    rdt = real_dtype(a.dtype)
    check("dlaf_mi355x_hermitian_rank_k_update_device", uplo.encode(), trans.encode(), scalar(alpha, rdt), a._h,
          scalar(beta, rdt), c._h)


def hermitian_rank_2k_update_device(uplo: str, trans: str, alpha, a: GeneralDeviceMatrix, b: GeneralDeviceMatrix, beta,
                                    c: DeviceMatrix) -> None:
    """hermitian_rank_2k_update on resident operands (`a`, `b` general resident matrices as stored, `c` a DeviceMatrix
    created with this uplo); only the uplo triangle of `c` is written; no PCIe traffic."""
    check("dlaf_mi355x_hermitian_rank_2k_update_device", uplo.encode(), trans.encode(), scalar(alpha, a.dtype), a._h, b._h,
          scalar(beta, real_dtype(a.dtype)), c._h)
