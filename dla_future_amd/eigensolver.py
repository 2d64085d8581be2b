"""First stage of the Hermitian eigensolver: reduction to band and its back-transformation.

Mirrors dlaf::eigensolver::internal::reduction_to_band (include/dlaf/eigensolver/reduction_to_band.h:40-122) and
bt_reduction_to_band (include/dlaf/eigensolver/bt_reduction_to_band.h) over the C ABI
(dlaf_mi355x_reduction_to_band_*, dlaf_mi355x_bt_reduction_to_band_*).  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (check_stage, desc9, descriptor, entry, global_size, global_sizes, ld_of, make_descriptor, ptr, real_dtype,
                   two_doubles)
from .capi import lib, type_char
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def get_band_size(nb: int) -> int:
    """include/dlaf/eigensolver/internal/get_band_size.h:20-31 with the tune parameter eigensolver_min_band."""
    return lib().dlaf_mi355x_get_band_size(nb)


def red2band_panel_stats():
    """(blocked, fallback): panels of this process's last reduction_to_band factored by the blocked path / handed back to
    the reflector-by-reflector kernel."""
    a, b = C.c_long(0), C.c_long(0)
    lib().dlaf_mi355x_red2band_panel_stats(C.byref(a), C.byref(b))
    return a.value, b.value


def eigensolver_min_band(b_min: int | None = None) -> int:
    """getTuneParameters().eigensolver_min_band (include/dlaf/tune.h:128; DLAF_EIGENSOLVER_MIN_BAND, src/init.cpp:220):
    returns the current value, after setting it when `b_min` is given."""
    if b_min is not None:
        lib().dlaf_mi355x_set_eigensolver_min_band(int(b_min))
    return lib().dlaf_mi355x_get_eigensolver_min_band()


def reduction_to_band(grid: Grid, a: np.ndarray, nb: int, band_size: int, isrc: int = 0, jsrc: int = 0,
                      n: int | None = None) -> np.ndarray:
    """reduction_to_band(grid, mat_a, band_size): `a` (this process's local part; lower triangle referenced) is
    overwritten with the band and the Householder reflectors below it; returns taus (n - band_size - 1 values, all
    of them on every process)."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    taus = np.zeros(max(0, n - band_size - 1), dtype=a.dtype)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    check_stage(f"dlaf_mi355x_reduction_to_band_{t}", grid.context, ptr(a), da, band_size, ptr(taus))
    return taus


def bt_reduction_to_band(grid: Grid, band_size: int, c: np.ndarray, v: np.ndarray, taus: np.ndarray, nb: int, isrc: int = 0,
                         jsrc: int = 0, c_jsrc: int = 0, n: int | None = None, k: int | None = None) -> None:
    """bt_reduction_to_band(grid, band_size, mat_c, mat_v, taus): c (local part of the n x k matrix) <- Q c."""
    t = type_char(c.dtype)
    n, k = global_sizes(grid, (n, k), lambda: (v.shape[0], c.shape[1]), "global sizes n, k are")
    dc = descriptor(n, k, nb, (isrc, c_jsrc), ld_of(c))
    dv = make_descriptor(n, nb, ld_of(v), isrc, jsrc)
    check_stage(f"dlaf_mi355x_bt_reduction_to_band_{t}", grid.context, band_size, ptr(c), dc, ptr(v), dv, ptr(taus))


def reduction_to_band_device(a: DeviceMatrix, band_size: int) -> np.ndarray:
    """The same on a resident matrix (uplo 'L'); returns taus."""
    taus = np.zeros(max(0, a.n - band_size - 1), dtype=a.dtype)
    check_stage("dlaf_mi355x_reduction_to_band_device", a._h, band_size, ptr(taus))
    return taus


def bt_reduction_to_band_device(band_size: int, c: GeneralDeviceMatrix, v: DeviceMatrix, taus: np.ndarray) -> None:
    check_stage("dlaf_mi355x_bt_reduction_to_band_device", band_size, c._h, v._h, ptr(taus))


def red2band_profile():
    """(device ms, whole-grid algorithmic flops) of the last reduction_to_band / bt_reduction_to_band here."""
    return two_doubles("dlaf_mi355x_red2band_profile")


# ---- the stages behind reduction_to_band and the eigensolver drivers --------------------------------------------
def band_to_tridiagonal(grid: Grid, a: np.ndarray, nb: int, band_size: int, isrc: int = 0, jsrc: int = 0,
                        n: int | None = None):
    """band_to_tridiagonal<Backend::MC>(grid, Lower, band_size, mat_a) (include/dlaf/eigensolver/band_to_tridiag.h:74-176):
    `a` holds a Hermitian band matrix in the lower band of its local part.  Returns (d, e, v): the diagonal (n), the
    off-diagonal (n - 1, real) and the n x n matrix of compact Householder reflectors (tau in the place of the leading
    1, band_to_tridiag.h:40-72) -- complete on every process."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    rt = real_dtype(a.dtype)
    d = np.zeros(n, dtype=rt)
    e = np.zeros(n, dtype=rt)
    v = np.zeros((n, n), dtype=a.dtype, order="F")
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    check_stage(f"dlaf_mi355x_band_to_tridiagonal_{t}", grid.context, ptr(a), da, band_size, ptr(d), ptr(e), ptr(v), max(1, n))
    return d, e[:max(n - 1, 0)].copy(), v


def bt_band_to_tridiagonal(band_size: int, e: np.ndarray, v: np.ndarray) -> None:
    """bt_band_to_tridiagonal(band_size, mat_e, mat_hh) (include/dlaf/eigensolver/bt_band_to_tridiag.h:28-61), local:
    e (n x k, column-major) <- Q e."""
    t = type_char(e.dtype)
    n, k = e.shape
    check_stage(f"dlaf_mi355x_bt_band_to_tridiagonal_{t}", band_size, n, k, ptr(v), ld_of(v), ptr(e), ld_of(e))


def _index_range(eigenvalues_index, n):
    begin, end = eigenvalues_index
    return int(begin), int(end)


def tridiagonal_eigensolver(d: np.ndarray, e: np.ndarray, nb: int = 512, eigenvalues_index=None, z: np.ndarray | None = None):
    """tridiagonal_eigensolver(tridiag, evals, evecs) (include/dlaf/eigensolver/tridiag_solver.h:30-60), local:
    returns (w ascending, z column-major n x n).  eigenvalues_index = (begin, end): only the eigenvectors of the
    eigenvalues [begin, end) (0-based, half-open) are computed and z is n x (end - begin); w still holds all n
    eigenvalues.  z: a preallocated column-major array to write into (only its leading n x (end - begin) block is)."""
    t = type_char(d.dtype)
    n = d.shape[0]
    d = np.ascontiguousarray(d)
    e = np.ascontiguousarray(e, dtype=d.dtype)
    w = np.zeros(n, dtype=d.dtype)
    if eigenvalues_index is not None:
        begin, end = _index_range(eigenvalues_index, n)
        if z is None:
            z = np.zeros((n, max(end - begin, 0)), dtype=d.dtype, order="F")
        check_stage(f"dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_{t}", n, nb, ptr(d), ptr(e), ptr(w), ptr(z),
                    ld_of(z), begin, end)
        return w, z
    z = np.zeros((n, n), dtype=d.dtype, order="F")
    check_stage(f"dlaf_mi355x_tridiagonal_eigensolver_{t}", n, nb, ptr(d), ptr(e), ptr(w), ptr(z), max(1, n))
    return w, z


def _eig_name(t: str) -> str:
    return "symmetric" if t in "sd" else "hermitian"


def _one_selection(eigenvalues_index, eigenvalues_value):
    if eigenvalues_index is not None and eigenvalues_value is not None:
        raise ValueError("eigenvalues_index and eigenvalues_value are mutually exclusive")


# ---- eigenvalues only: bisection on Sturm counts of the tridiagonal matrix ------------------
def sturm_layout():
    """(pairs of the tridiagonal matrix staged through LDS at a time, threads per workgroup) of the Sturm kernels."""
    out = (C.c_int * 2)()
    lib().dlaf_mi355x_sturm_layout(out)
    return out[0], out[1]


def tridiagonal_eigenvalues(d: np.ndarray, e: np.ndarray, eigenvalues_index=None, w: np.ndarray | None = None):
    """Eigenvalues of the symmetric tridiagonal matrix d (n), e (n - 1) by bisection on Sturm counts, local, on the GPU:
    no eigenvectors, O(n) memory.  eigenvalues_index = (begin, end): only w[begin:end] is computed and written (0-based,
    half-open; default all n).  w: a preallocated array to write into.  Returns w (ascending)."""
    t = type_char(d.dtype)
    n = d.shape[0]
    d = np.ascontiguousarray(d)
    e = np.ascontiguousarray(e, dtype=d.dtype)
    if w is None:
        w = np.zeros(n, dtype=d.dtype)
    begin, end = (0, n) if eigenvalues_index is None else _index_range(eigenvalues_index, n)
    check_stage(f"dlaf_mi355x_tridiagonal_eigenvalues_{t}", n, ptr(d), ptr(e), ptr(w), begin, end)
    return w


def tridiagonal_sturm_count(d: np.ndarray, e: np.ndarray, shifts) -> np.ndarray:
    """counts[i] = the number of eigenvalues of the symmetric tridiagonal matrix d, e that are <= shifts[i] (LAPACK
    dstebz's convention), one GPU thread per shift.  -1 for every shift when d or e holds a NaN or an Inf."""
    t = type_char(d.dtype)
    n = d.shape[0]
    d = np.ascontiguousarray(d)
    e = np.ascontiguousarray(e, dtype=d.dtype)
    shifts = np.ascontiguousarray(shifts, dtype=d.dtype).reshape(-1)
    counts = np.zeros(shifts.shape[0], dtype=np.int64)
    check_stage(f"dlaf_mi355x_tridiagonal_sturm_count_{t}", n, ptr(d), ptr(e), shifts.shape[0], ptr(shifts), ptr(counts))
    return counts


def hermitian_eigenvalues(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                          n: int | None = None, eigenvalues_index=None, w: np.ndarray | None = None) -> np.ndarray:
    """Eigenvalues only (dlaf_{symmetric,hermitian}_eigenvalues_*): reduction_to_band, band_to_tridiagonal and bisection
    for the eigenvalues eigenvalues_index = [begin, end) (default all n).  No divide & conquer, no back-transformation,
    no eigenvector matrix.  `a` (local part, the uplo triangle referenced) is not modified.  Only w[begin:end] is
    written (w: a preallocated array of n reals); returns w."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    if w is None:
        w = np.zeros(n, dtype=real_dtype(a.dtype))
    begin, end = (0, n) if eigenvalues_index is None else _index_range(eigenvalues_index, n)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    check_stage(f"dlaf_{_eig_name(t)}_eigenvalues_{t}", grid.context, uplo.encode()[0:1], ptr(a), da, ptr(w), begin, end)
    return w


def hermitian_generalized_eigenvalues(grid: Grid, uplo: str, a: np.ndarray, b: np.ndarray, nb: int, isrc: int = 0,
                                      jsrc: int = 0, n: int | None = None, factorized: bool = False,
                                      eigenvalues_index=None, w: np.ndarray | None = None) -> np.ndarray:
    """Eigenvalues only of A x = lambda B x (dlaf_{symmetric,hermitian}_generalized_eigenvalues[_factorized]_*):
    Cholesky of b (unless factorized), generalized_to_standard, then as hermitian_eigenvalues.  b ends up holding its
    Cholesky factor."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    if w is None:
        w = np.zeros(n, dtype=real_dtype(a.dtype))
    begin, end = (0, n) if eigenvalues_index is None else _index_range(eigenvalues_index, n)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    db = make_descriptor(n, nb, ld_of(b), isrc, jsrc)
    check_stage(f"dlaf_{_eig_name(t)}_generalized_eigenvalues{'_factorized' if factorized else ''}_{t}", grid.context,
                uplo.encode()[0:1], ptr(a), da, ptr(b), db, ptr(w), begin, end)
    return w


def _solve(stem: str, t: str, grid, uplo, operands, n, w, z, dz, eigenvalues_index, eigenvalues_value):
    """The three forms of a driver: all eigenpairs, <stem>_partial_spectrum and <stem>_partial_spectrum_by_value."""
    head = (grid.context, uplo.encode()[0:1], *operands, ptr(w), ptr(z), dz)
    if eigenvalues_value is not None:
        begin, end = C.c_long(-1), C.c_long(-1)
        check_stage(f"{stem}_partial_spectrum_by_value_{t}", *head, float(eigenvalues_value[0]), float(eigenvalues_value[1]),
                    C.byref(begin), C.byref(end))
        return w, z, (begin.value, end.value)
    if eigenvalues_index is None:
        check_stage(f"{stem}_{t}", *head)
    else:
        check_stage(f"{stem}_partial_spectrum_{t}", *head, *_index_range(eigenvalues_index, n))
    return w, z


def hermitian_eigensolver(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                          n: int | None = None, z_jsrc: int | None = None, z_shape=None, eigenvalues_index=None,
                          z: np.ndarray | None = None, eigenvalues_value=None):
    """dlaf::hermitian_eigensolver(grid, uplo, mat_a, evals, evecs) through the reference's C entry
    dlaf_{symmetric,hermitian}_eigensolver_* (include/dlaf_c/eigensolver/eigensolver.h:39-58).  `a` (local part, the uplo
    triangle referenced) is destroyed.  Returns (w, z): all eigenvalues (ascending) and the local part of the
    eigenvector matrix.

    eigenvalues_index = (begin, end): the *_partial_spectrum entry -- only the global columns [begin, end) of z (0-based,
    half-open) are written, with the eigenvectors of those eigenvalues; w still holds all n.  z: a preallocated
    column-major local part to write into (nothing outside the wanted columns is touched).

    eigenvalues_value = (vl, vu): the *_partial_spectrum_by_value entry -- the eigenpairs with eigenvalues in (vl, vu].
    Returns (w, z, (begin, end)): the index range the two Sturm counts of the tridiagonal matrix gave, and otherwise what
    eigenvalues_index=(begin, end) returns.  An eigenvalue within rounding of vl or vu may fall on either side."""
    t = type_char(a.dtype)
    _one_selection(eigenvalues_index, eigenvalues_value)
    n = global_size(grid, n, a)
    if z_jsrc is None:
        z_jsrc = jsrc
    w = np.zeros(n, dtype=real_dtype(a.dtype))
    if z is None:
        z = np.zeros(z_shape if z_shape is not None else a.shape, dtype=a.dtype, order="F")
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    dz = make_descriptor(n, nb, ld_of(z), isrc, z_jsrc)
    return _solve(f"dlaf_{_eig_name(t)}_eigensolver", t, grid, uplo, (ptr(a), da), n, w, z, dz, eigenvalues_index,
                  eigenvalues_value)


def hermitian_generalized_eigensolver(grid: Grid, uplo: str, a: np.ndarray, b: np.ndarray, nb: int, isrc: int = 0,
                                      jsrc: int = 0, n: int | None = None, factorized: bool = False,
                                      eigenvalues_index=None, z: np.ndarray | None = None, eigenvalues_value=None):
    """dlaf::hermitian_generalized_eigensolver(grid, uplo, mat_a, mat_b, evals, evecs) through the reference's C entry
    (include/dlaf_c/eigensolver/gen_eigensolver.h:44-135).  a is destroyed, b ends up holding its Cholesky factor.
    eigenvalues_index, z, eigenvalues_value: as in hermitian_eigensolver."""
    t = type_char(a.dtype)
    _one_selection(eigenvalues_index, eigenvalues_value)
    n = global_size(grid, n, a)
    w = np.zeros(n, dtype=real_dtype(a.dtype))
    if z is None:
        z = np.zeros(a.shape, dtype=a.dtype, order="F")
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    db = make_descriptor(n, nb, ld_of(b), isrc, jsrc)
    dz = make_descriptor(n, nb, ld_of(z), isrc, jsrc)
    return _solve(f"dlaf_{_eig_name(t)}_generalized_eigensolver{'_factorized' if factorized else ''}", t, grid, uplo,
                  (ptr(a), da, ptr(b), db), n, w, z, dz, eigenvalues_index, eigenvalues_value)


def eigensolver_profile():
    """device ms per stage of the last eigensolver call: reduction_to_band, band_to_tridiagonal, tridiagonal_eigensolver,
    bt_band_to_tridiagonal, bt_reduction_to_band."""
    ms = (C.c_double * 5)()
    lib().dlaf_mi355x_eigensolver_profile(ms)
    return list(ms)


def pxheevd_partial_spectrum(uplo: str, a: np.ndarray, desca, z: np.ndarray, descz, il: int, iu: int, n: int):
    """dlaf_p{s,d}syevd_partial_spectrum / dlaf_p{c,z}heevd_partial_spectrum: the ScaLAPACK-like argument list with the
    1-based inclusive index range (il, iu) of p?syevx in front of info ((1, 0): the empty range).  desca, descz: the nine
    integers of the ScaLAPACK descriptors.  Returns (w, info); z is written in place."""
    t = type_char(a.dtype)
    name = f"dlaf_p{t}{'syevd' if t in 'sd' else 'heevd'}_partial_spectrum"
    w = np.zeros(n, dtype=real_dtype(a.dtype))
    da = desc9(desca)
    dz = desc9(descz)
    info = C.c_int(-1)
    entry(name)(uplo.encode()[0:1], n, ptr(a), 1, 1, da, ptr(w), ptr(z), 1, 1, dz, il, iu, C.byref(info))
    return w, info.value


def pxheevd_eigenvalues(uplo: str, a: np.ndarray, desca, il: int, iu: int, n: int, w: np.ndarray | None = None):
    """dlaf_p{s,d}syevd_eigenvalues / dlaf_p{c,z}heevd_eigenvalues: eigenvalues only through the ScaLAPACK-like argument
    list, 1-based inclusive (il, iu) in front of info.  Returns (w, info); only w[il - 1:iu] is written."""
    t = type_char(a.dtype)
    name = f"dlaf_p{t}{'syevd' if t in 'sd' else 'heevd'}_eigenvalues"
    if w is None:
        w = np.zeros(n, dtype=real_dtype(a.dtype))
    da = desc9(desca)
    info = C.c_int(-1)
    entry(name)(uplo.encode()[0:1], n, ptr(a), 1, 1, da, ptr(w), il, iu, C.byref(info))
    return w, info.value


def pxheevd_partial_spectrum_by_value(uplo: str, a: np.ndarray, desca, z: np.ndarray, descz, vl: float, vu: float, n: int):
    """dlaf_p{s,d}syevd_partial_spectrum_by_value / dlaf_p{c,z}heevd_partial_spectrum_by_value: the eigenpairs in
    (vl, vu] through the ScaLAPACK-like argument list, with vl, vu, m in front of info.  Returns (w, m, info); z is
    written in place (m columns, from the column of the first eigenvalue above vl)."""
    t = type_char(a.dtype)
    name = f"dlaf_p{t}{'syevd' if t in 'sd' else 'heevd'}_partial_spectrum_by_value"
    w = np.zeros(n, dtype=real_dtype(a.dtype))
    da = desc9(desca)
    dz = desc9(descz)
    m, info = C.c_int(-1), C.c_int(-1)
    entry(name)(uplo.encode()[0:1], n, ptr(a), 1, 1, da, ptr(w), ptr(z), 1, 1, dz, float(vl), float(vu),
                         C.byref(m), C.byref(info))
    return w, m.value, info.value


def _gv_name(t: str) -> str:
    return f"dlaf_p{t}{'sygvd' if t in 'sd' else 'hegvd'}"


def pxhegvd_eigenvalues(uplo: str, a: np.ndarray, desca, b: np.ndarray, descb, il: int, iu: int, n: int,
                        factorized: bool = False, w: np.ndarray | None = None):
    """dlaf_p{s,d}sygvd_eigenvalues[_factorized] / dlaf_p{c,z}hegvd_eigenvalues[_factorized]: eigenvalues only of
    A x = lambda B x through the ScaLAPACK-like argument list.  Returns (w, info); only w[il - 1:iu] is written."""
    t = type_char(a.dtype)
    name = _gv_name(t) + "_eigenvalues" + ("_factorized" if factorized else "")
    if w is None:
        w = np.zeros(n, dtype=real_dtype(a.dtype))
    info = C.c_int(-1)
    entry(name)(uplo.encode()[0:1], n, ptr(a), 1, 1, desc9(desca), ptr(b), 1, 1, desc9(descb),
                         ptr(w), il, iu, C.byref(info))
    return w, info.value


def pxhegvd_partial_spectrum_by_value(uplo: str, a: np.ndarray, desca, b: np.ndarray, descb, z: np.ndarray, descz,
                                      vl: float, vu: float, n: int, factorized: bool = False):
    """dlaf_p{s,d}sygvd[_factorized]_partial_spectrum_by_value / dlaf_p{c,z}hegvd[_factorized]_partial_spectrum_by_value.
    Returns (w, m, info); z is written in place."""
    t = type_char(a.dtype)
    name = _gv_name(t) + ("_factorized" if factorized else "") + "_partial_spectrum_by_value"
    w = np.zeros(n, dtype=real_dtype(a.dtype))
    m, info = C.c_int(-1), C.c_int(-1)
    entry(name)(uplo.encode()[0:1], n, ptr(a), 1, 1, desc9(desca), ptr(b), 1, 1, desc9(descb),
                         ptr(w), ptr(z), 1, 1, desc9(descz), float(vl), float(vu), C.byref(m), C.byref(info))
    return w, m.value, info.value


def partial_spectrum_plan(n: int, nb: int, npcol: int, mycol: int, z_jsrc: int, begin: int, end: int):
    """dlaf_mi355x_partial_spectrum_plan (host only): (b0, column source rank of the internal eigenvector matrix, its
    local columns on process column mycol, the caller's local column its first one corresponds to, leading pad columns)."""
    out = (C.c_long * 5)()
    lib().dlaf_mi355x_partial_spectrum_plan(n, nb, npcol, mycol, z_jsrc, begin, end, out)
    return tuple(out)
