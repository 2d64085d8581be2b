"""Max, one, infinity and Frobenius norms on the grid (dlaf_mi355x_{general,hermitian,triangular}_norm_*,
dlaf_mi355x_p?lange, p?lansy / p?lanhe, p?lantr; csrc/host/norm.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import desc9, descriptor, entry, global_sizes, ld_of, ptr, two_doubles
from .capi import lib, type_char
from .device_matrix import GeneralDeviceMatrix
from .grid import Grid

NORM_ERRORS = {-1: "bad norm letter", -2: "bad uplo", -3: "bad diag", -4: "bad descriptor", -5: "source process outside the grid",
               -6: "missing value or context"}


def _value(who: str, r: int, v: C.c_double) -> float:
    if r != 0:
        raise ValueError(f"{who} failed with {r}: {NORM_ERRORS.get(r, '?')}")
    return v.value


def matrix_norm(grid: Grid, norm: str, a: np.ndarray, nb: int, structure: str = "G", uplo: str = "L", diag: str = "N",
                m: int | None = None, n: int | None = None, isrc: int = 0, jsrc: int = 0) -> float:
    """dlaf::auxiliary::max_norm and its one / infinity / Frobenius siblings == dlaf_mi355x_{general,hermitian,
    triangular}_norm_{s,d,c,z} (LAPACK xLANGE, xLANHE / xLANSY, xLANTR).  norm: 'M', '1' / 'O', 'I', 'F' / 'E';
    structure 'G' (the m x n matrix), 'H' (Hermitian from the uplo triangle) or 'T' (triangular, diag 'N' / 'U').
    `a`: this process's local column-major part, only read.  The value is the same on every rank."""
    t = type_char(a.dtype)
    m, n = global_sizes(grid, (m, n), a.shape, "the global size m x n is")
    da = descriptor(m, n, nb, (isrc, jsrc), ld_of(a))
    s = structure.upper()
    if s == "G":
        kind, letters = "general", (norm,)
    elif s in ("H", "S"):
        kind, letters = "hermitian", (norm, uplo)
    elif s == "T":
        kind, letters = "triangular", (norm, uplo, diag)
    else:
        raise ValueError(f"structure must be 'G', 'H' or 'T', got {structure!r}")
    v = C.c_double(-1.0)
    r = entry(f"dlaf_mi355x_{kind}_norm_{t}")(grid.context, *(x.encode() for x in letters), ptr(a), da, C.byref(v))
    return _value("matrix_norm", r, v)


def matrix_norm_device(norm: str, A, structure: str | None = None, diag: str = "N") -> float:
    """The norm of a resident operand, no PCIe traffic but the value: a GeneralDeviceMatrix (structure None / 'G') or the
    triangle a DeviceMatrix holds, read as Hermitian ('H', the default) or triangular ('T', diag 'N' / 'U')."""
    v = C.c_double(-1.0)
    if isinstance(A, GeneralDeviceMatrix):
        if structure not in (None, "G", "g"):
            raise ValueError("a GeneralDeviceMatrix is a general matrix")
        r = lib().dlaf_mi355x_general_matrix_norm(A._h, norm.encode(), C.byref(v))
    else:
        r = lib().dlaf_mi355x_matrix_norm(A._h, norm.encode(), (structure or "H").encode(), diag.encode(), C.byref(v))
    return _value("matrix_norm_device", r, v)


def _scalapack(routine: str, letters, sizes, a, ia, ja, desca) -> float:
    """dlaf_mi355x_p{s,d,c,z}<routine>: ScaLAPACK's argument list without work."""
    return float(entry(f"dlaf_mi355x_p{type_char(a.dtype)}{routine}")(*(x.encode() for x in letters), *sizes, ptr(a), ia, ja,
                                                                      desc9(desca)))


def pxlange(norm: str, m: int, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{s,d,c,z}lange: ScaLAPACK's p?lange argument list without work; returns the value."""
    return _scalapack("lange", (norm,), (m, n), a, ia, ja, desca)


def pxlanhe(norm: str, uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{c,z}lanhe / p{s,d}lansy: ScaLAPACK's argument list without work; returns the value."""
    return _scalapack("lanhe" if type_char(a.dtype) in "cz" else "lansy", (norm, uplo), (n,), a, ia, ja, desca)


def pxlantr(norm: str, uplo: str, diag: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{s,d,c,z}lantr: ScaLAPACK's p?lantr argument list without work; returns the value."""
    return _scalapack("lantr", (norm, uplo, diag), (n,), a, ia, ja, desca)


def norm_profile():
    """(ms, bytes) of the last norm on this process: device time (no upload) and the bytes of the tiles it referenced
    (diagonal tiles counted whole)."""
    return two_doubles("dlaf_mi355x_norm_profile")
