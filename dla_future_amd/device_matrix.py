"""The two resident matrix classes: DeviceMatrix (one triangle of a square matrix, what the factorization takes) and
GeneralDeviceMatrix (m x n), both in HBM in tile layout (dlaf_mi355x_matrix_*, dlaf_mi355x_gmatrix_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import check, descriptor, ld_of, make_descriptor, ptr
from .capi import lib, type_char
from .grid import Grid


class DeviceMatrix:
    """Matrix<T, Device::GPU> of the MI355X build: the local part of a block-cyclic matrix resident
    in HBM in tile layout (reference: matrix/matrix.h:57-357 + MatrixMirror, matrix_mirror.h:137-173).
    A driver uploads once and times `factorize` alone, like miniapp_cholesky.cpp:133-155."""

    def __init__(self, grid: Grid, dtype, uplo: str, n: int, nb: int, isrc: int = 0, jsrc: int = 0):
        self.grid, self.dtype, self.uplo, self.n, self.nb = grid, np.dtype(dtype), uplo, n, nb
        self._h = C.c_void_p()
        desc = make_descriptor(n, nb, 1, isrc, jsrc)
        check("dlaf_mi355x_matrix_create", grid.context, type_char(dtype).encode(), uplo.encode(), desc, C.byref(self._h))

    def upload(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_matrix_upload(self._h, ptr(a), ld_of(a))

    def download(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_matrix_download(self._h, ptr(a), ld_of(a))

    def fetch_tile(self, gi: int, gj: int):
        """Global tile (gi, gj) of the device copy as a dense column-major array, or None when this process
        does not own it (a checker samples a large factor tile by tile instead of downloading it whole)."""
        rows = min(self.nb, self.n - gi * self.nb)
        cols = min(self.nb, self.n - gj * self.nb)
        out = np.zeros((rows, cols), dtype=self.dtype, order="F")
        r = lib().dlaf_mi355x_matrix_fetch_tile(self._h, gi, gj, ptr(out), max(1, rows))
        if r < 0:
            raise ValueError(f"dlaf_mi355x_matrix_fetch_tile failed with {r}")
        return out if r == 0 else None

    def copy_from(self, other: "DeviceMatrix") -> None:
        r = lib().dlaf_mi355x_matrix_copy(self._h, other._h)
        if r != 0:
            raise ValueError("matrices are not conformable")

    def factorize(self) -> int:
        """dlaf::cholesky_factorization<Backend::GPU, Device::GPU, T> on the resident matrix; blocking."""
        return lib().dlaf_mi355x_cholesky_factorization_device(self._h)

    def generalized_to_standard(self, factor_of_b: "DeviceMatrix") -> int:
        """`self` (Hermitian A, resident) <- inv(L) A inv(L^H) with the resident Cholesky factor of B."""
        return lib().dlaf_mi355x_generalized_to_standard_device(self._h, factor_of_b._h)

    def invert_triangular(self, diag: str = "N") -> int:
        """The resident triangular matrix (this matrix's uplo triangle) <- its inverse; returns LAPACK's info."""
        return lib().dlaf_mi355x_triangular_inverse_device(self.uplo.encode(), diag.encode(), self._h)

    def invert_from_factor(self) -> int:
        """The resident Cholesky factor <- the uplo triangle of inv(L L^H) / inv(U^H U); returns LAPACK's info."""
        return lib().dlaf_mi355x_inverse_from_cholesky_factor_device(self.uplo.encode(), self._h)

    def to_general(self, g: "GeneralDeviceMatrix", kind: str = "H") -> None:
        """Writes into the resident general matrix `g` (same grid, type, n x n, block and source process) the Hermitian
        (kind 'H') / symmetric ('S') matrix whose uplo triangle this matrix holds, or the triangular one ('T': exact
        zeros in the other triangle), as download() of `g` shows it; nothing crosses PCIe."""
        check("dlaf_mi355x_matrix_to_general", kind.encode(), self._h, g._h)

    def from_general(self, g: "GeneralDeviceMatrix") -> None:
        """Takes this matrix's uplo triangle from the resident general matrix `g`; nothing crosses PCIe."""
        check("dlaf_mi355x_matrix_from_general", self._h, g._h)

    def start(self) -> None:
        lib().dlaf_mi355x_cholesky_start(self._h)

    def wait(self) -> int:
        return lib().dlaf_mi355x_cholesky_wait(self._h)

    def local_info(self) -> int:
        """This process's own device status word of the last factorization, before the grid agreed on one value."""
        return lib().dlaf_mi355x_matrix_local_info(self._h)

    def residual_against(self, factor: "DeviceMatrix"):
        """check_cholesky of the miniapp (miniapp_cholesky.cpp:408-443) on the device.  `self` must hold the
        ORIGINAL matrix and is overwritten with A - L L^H.  Returns (max|A - L L^H|, max|A|) over the grid."""
        d, a = C.c_double(), C.c_double()
        r = lib().dlaf_mi355x_cholesky_residual(self._h, factor._h, C.byref(d), C.byref(a))
        if r != 0:
            raise ValueError("matrices are not conformable")
        return d.value, a.value

    PROFILE_KINDS = {"update_bulk": 0, "update_lookahead": 1, "trsm_panel": 2, "potrf_tile": 3}

    def profile(self, kind: str) -> dict:
        """HIP-event timing of one launch class of the last factorization (after wait())."""
        ms, n, fl, by = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib().dlaf_mi355x_matrix_profile(self._h, self.PROFILE_KINDS[kind], C.byref(ms), C.byref(n), C.byref(fl),
                                         C.byref(by))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    def trsm_profile(self, reps: int = 5) -> dict:
        """The panel TRSM of step 0 alone on the device (after factorize(); one-process grids): HIP-event time per
        launch and the algorithmic work of one launch."""
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        lib().dlaf_mi355x_matrix_trsm_profile(self._h, reps, C.byref(ms), C.byref(fl), C.byref(by))
        return {"ms": ms.value, "flops": fl.value, "bytes": by.value}

    def close(self) -> None:
        if self._h:
            lib().dlaf_mi355x_matrix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GeneralDeviceMatrix:
    """A general m x n matrix resident in HBM in tile layout (square blocks): the right-hand sides of a
    device-resident solve (dlaf_mi355x_gmatrix_*)."""

    def __init__(self, grid: Grid, dtype, m: int, n: int, nb: int, isrc: int = 0, jsrc: int = 0):
        self.grid, self.dtype, self.m, self.n, self.nb = grid, np.dtype(dtype), m, n, nb
        self._h = C.c_void_p()
        desc = descriptor(m, n, nb, (isrc, jsrc), 1)
        check("dlaf_mi355x_gmatrix_create", grid.context, type_char(dtype).encode(), desc, C.byref(self._h))

    def upload(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_gmatrix_upload(self._h, ptr(a), ld_of(a))

    def download(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_gmatrix_download(self._h, ptr(a), ld_of(a))

    def close(self) -> None:
        if self._h:
            lib().dlaf_mi355x_gmatrix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
