"""The weighted Hermitian rank-k update C = alpha A D A^H + beta C and the functions of a Hermitian matrix built on it
(dlaf_mi355x_hermitian_weighted_rank_k_update_*, dlaf_mi355x_hermitian_function_*, dlaf_mi355x_hermitian_power_*;
csrc/host/rank_update.cpp, csrc/host/matrix_function.cpp).  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (check, check_stage, descriptor, entry, global_size, global_sizes, ld_of, make_descriptor, ptr, real_dtype,
                   scalar)
from .capi import WEIGHTS_FN_D, WEIGHTS_FN_S, lib, type_char
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix
from .grid import Grid


def _weights_ptr(d, k, rdt):
    """the k real weights as a contiguous array of the real type (None stays None: the entry judges it); the pointer
    keeps the array alive"""
    if d is None:
        return None
    d = np.ascontiguousarray(d, dtype=rdt).reshape(-1)
    if d.shape[0] != k:
        raise ValueError(f"d holds {d.shape[0]} weights, k is {k}")
    return ptr(d)


def hermitian_weighted_rank_k_update(grid: Grid, uplo: str, trans: str, alpha, a: np.ndarray, d, beta, c: np.ndarray,
                                     nb: int, n: int | None = None, k: int | None = None, a_src=(0, 0),
                                     c_src=(0, 0)) -> None:
    """"xSYRK / xHERK with weights" == dlaf_mi355x_hermitian_weighted_rank_k_update_{s,d,c,z}: the uplo triangle of the
    n x n matrix C becomes alpha A D A^H + beta C (trans 'N', A stored n x k) or alpha A^H D A + beta C (trans 'C', A
    stored k x n) with D = diag(d), d: k REAL weights of any sign (the same on every rank); alpha and beta are real.  The
    weights are multiplied into one operand inside the rank-k kernel: no scaled copy of A, the flops of a rank-k update.
    Otherwise as hermitian_rank_k_update (the other triangle is never referenced, the diagonal comes back real, beta = 0
    does not read C, alpha = 0 or k = 0 reference neither A nor d).  A zero weight does NOT unreference its column:
    0 * NaN is NaN."""
    t = type_char(c.dtype)
    if a.dtype != c.dtype:
        raise ValueError("the operands must have the same element type")
    tn = trans.upper() == "N"
    n, k = global_sizes(grid, (n, k), lambda: (c.shape[0], a.shape[1] if tn else a.shape[0]), "the global sizes n, k are")
    rdt = real_dtype(c.dtype)
    da = descriptor(n if tn else k, k if tn else n, nb, a_src, ld_of(a))
    dc = descriptor(n, n, nb, c_src, ld_of(c))
    check(f"dlaf_mi355x_hermitian_weighted_rank_k_update_{t}", grid.context, uplo.encode(), trans.encode(), scalar(alpha, rdt),
          ptr(a), da, _weights_ptr(d, k, rdt), scalar(beta, rdt), ptr(c), dc)


def hermitian_weighted_rank_k_update_device(uplo: str, trans: str, alpha, a: GeneralDeviceMatrix, d, beta,
                                            c: DeviceMatrix) -> None:
    """hermitian_weighted_rank_k_update on resident operands: `c` a DeviceMatrix created with this uplo, `a` a general
    resident matrix as stored, `d` the k real weights on the host; only the uplo triangle of `c` is written."""
    rdt = real_dtype(a.dtype)
    k = a.n if trans.upper() == "N" else a.m
    check("dlaf_mi355x_hermitian_weighted_rank_k_update_device", uplo.encode(), trans.encode(), scalar(alpha, rdt), a._h,
          _weights_ptr(d, k, rdt), scalar(beta, rdt), c._h)


def _weights_callback(fn, rdt):
    """`fn`: ndarray of eigenvalues -> ndarray of weights, behind dlaf_mi355x_spectral_weights_{s,d}.  It is handed the
    selected eigenvalues w[begin:end] and its result fills g[begin:end]; an exception it raises is kept and raised again
    once the library has returned (the weights are zero then)."""
    failure = []

    def call(n, w, begin, end, g, user):
        try:
            if end > begin:
                lam = np.ctypeslib.as_array(w, shape=(n,))[begin:end].copy()
                out = np.asarray(fn(lam), dtype=rdt).reshape(-1)
                if out.shape[0] != end - begin:
                    raise ValueError(f"fn returned {out.shape[0]} weights for {end - begin} eigenvalues")
                np.ctypeslib.as_array(g, shape=(n,))[begin:end] = out
        except Exception as e:  # (no exception may cross the C frames)
            failure.append(e)

    cb = (WEIGHTS_FN_S if rdt == np.float32 else WEIGHTS_FN_D)(call)
    return cb, failure


def _selection(eigenvalues_index, eigenvalues_value, rdt):
    if eigenvalues_index is not None and eigenvalues_value is not None:
        raise ValueError("eigenvalues_index and eigenvalues_value are mutually exclusive")
    idx = None if eigenvalues_index is None else np.array([int(eigenvalues_index[0]), int(eigenvalues_index[1])], dtype=np.int64)
    val = None if eigenvalues_value is None else np.array([eigenvalues_value[0], eigenvalues_value[1]], dtype=rdt)
    return idx, val


def hermitian_function(grid: Grid, uplo: str, a: np.ndarray, nb: int, fn, isrc: int = 0, jsrc: int = 0,
                       n: int | None = None, eigenvalues_index=None, eigenvalues_value=None):
    """f(A) of a Hermitian matrix == dlaf_mi355x_hermitian_function_{s,d,c,z}: the uplo ('L') triangle of `a` (this
    process's local part) becomes that of sum_j fn(w)_j z_j z_j^H over the selected eigenpairs -- all (default),
    eigenvalues_index = (begin, end) or eigenvalues_value = (vl, vu], meaning vl < w <= vu.  `fn` maps an ndarray of the
    selected eigenvalues to an ndarray of their weights; unselected eigenvalues weigh 0 and their eigenvectors are never
    computed.  The eigenvectors never leave the GPU.  Returns (w, (begin, end)): all n eigenvalues and the selected range.
    Raises RuntimeError with the eigensolver's status when that is not 0 (`a` is unchanged then)."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    rdt = real_dtype(a.dtype)
    w = np.zeros(max(n, 1), dtype=rdt)
    idx, val = _selection(eigenvalues_index, eigenvalues_value, rdt)
    cb, failure = _weights_callback(fn, rdt)
    sel = np.zeros(2, dtype=np.int64)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    name = f"dlaf_mi355x_hermitian_function_{t}"
    r = entry(name)(grid.context, uplo.encode()[0:1], ptr(a), da, ptr(w), cb, None, ptr(idx), ptr(val), ptr(sel))
    if failure:
        raise failure[0]
    if r != 0:
        raise RuntimeError(f"{name} returned {r}")
    return w[:n], (int(sel[0]), int(sel[1]))


def hermitian_function_device(a: DeviceMatrix, fn, eigenvalues_index=None, eigenvalues_value=None):
    """hermitian_function on a resident matrix (created with uplo 'L'): A := f(A) in place, only the eigenvalues cross
    PCIe.  Returns (w, (begin, end))."""
    rdt = real_dtype(a.dtype)
    w = np.zeros(max(a.n, 1), dtype=rdt)
    idx, val = _selection(eigenvalues_index, eigenvalues_value, rdt)
    cb, failure = _weights_callback(fn, rdt)
    sel = np.zeros(2, dtype=np.int64)
    r = lib().dlaf_mi355x_hermitian_function_device(a._h, ptr(w), C.cast(cb, C.c_void_p), None, ptr(idx), ptr(val),
                                                    ptr(sel))
    if failure:
        raise failure[0]
    if r != 0:
        raise RuntimeError(f"dlaf_mi355x_hermitian_function_device returned {r}")
    return w[:a.n], (int(sel[0]), int(sel[1]))


def hermitian_power(grid: Grid, uplo: str, a: np.ndarray, nb: int, exponent: float, threshold: float = 0.0,
                    isrc: int = 0, jsrc: int = 0, n: int | None = None):
    """A^exponent of a Hermitian matrix on its eigenvalues above `threshold` (>= 0), the others dropped (weight 0: the
    pseudo-inverse for -1, Loewdin's S^(-1/2) for -0.5) == dlaf_mi355x_hermitian_power_{s,d,c,z}.  The dropped
    eigenvectors are not computed.  Returns (w, n_dropped)."""
    t = type_char(a.dtype)
    n = global_size(grid, n, a)
    w = np.zeros(max(n, 1), dtype=real_dtype(a.dtype))
    dropped = C.c_long(0)
    da = make_descriptor(n, nb, ld_of(a), isrc, jsrc)
    check_stage(f"dlaf_mi355x_hermitian_power_{t}", grid.context, uplo.encode()[0:1], ptr(a), da, ptr(w), float(exponent),
                float(threshold), C.byref(dropped))
    return w[:n], dropped.value


def hermitian_power_device(a: DeviceMatrix, exponent: float, threshold: float = 0.0):
    """hermitian_power on a resident matrix (created with uplo 'L'), in place.  Returns (w, n_dropped)."""
    w = np.zeros(max(a.n, 1), dtype=real_dtype(a.dtype))
    dropped = C.c_long(0)
    check_stage("dlaf_mi355x_hermitian_power_device", a._h, ptr(w), float(exponent), float(threshold), C.byref(dropped))
    return w[:a.n], dropped.value
