"""The tile operations with the argument sets the factorization issues, and the direct doors of the three kernels:
ONE launch each on flat host arrays (csrc/host/direct.hpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import entry, ld_of, ptr
from .capi import PotrfDesc, TrsmDesc, UpdateDesc, lib, type_char


def tile_potrf(uplo: str, a: np.ndarray) -> int:
    """tile::potrf (include/dlaf/lapack/tile.h:362-378); returns info."""
    return lib().dlaf_mi355x_tile_potrf(type_char(a.dtype).encode(), uplo.encode(), a.shape[0], ptr(a), ld_of(a))


def tile_trsm(uplo: str, a: np.ndarray, b: np.ndarray) -> None:
    """tile::trsm as cholesky/impl.h:56-67 (L: B <- B A^-H) / :110-121 (U: B <- A^-H B) call it."""
    m, n = b.shape
    lib().dlaf_mi355x_tile_trsm(type_char(b.dtype).encode(), uplo.encode(), m, n, ptr(a), ld_of(a), ptr(b),
                                ld_of(b))


def tile_herk(uplo: str, a: np.ndarray, c: np.ndarray) -> None:
    """tile::herk as impl.h:70-80 (L: C -= A A^H) / :124-134 (U: C -= A^H A) call it."""
    n = c.shape[0]
    k = a.shape[1] if uplo in "Ll" else a.shape[0]
    lib().dlaf_mi355x_tile_herk(type_char(c.dtype).encode(), uplo.encode(), n, k, ptr(a), ld_of(a), ptr(c),
                                ld_of(c))


def tile_gemm(uplo: str, a: np.ndarray, b: np.ndarray, c: np.ndarray) -> None:
    """tile::gemm as impl.h:83-94 (L: C -= A B^H) / :137-147 (U: C -= A^H B) call it."""
    m, n = c.shape
    k = a.shape[1] if uplo in "Ll" else a.shape[0]
    lib().dlaf_mi355x_tile_gemm(type_char(c.dtype).encode(), uplo.encode(), m, n, k, ptr(a), ld_of(a), ptr(b),
                                ld_of(b), ptr(c), ld_of(c))


def update_bulk_slots(dtype) -> int:
    """Workgroup slots of the bulk update kernel on this GPU for `dtype` (what the drivers size persistent launches by)."""
    return int(lib().dlaf_mi355x_update_bulk_slots(type_char(dtype).encode()))


def _descriptor(who: str, struct, arrays, fields, **preset):
    """The door's descriptor: the caller's `fields` over `preset`, once the operands are flat arrays of one dtype."""
    for x in arrays:
        if x is None or x.ndim != 1 or x.dtype != arrays[0].dtype or not x.flags.c_contiguous:
            raise ValueError(f"{who} takes flat contiguous arrays of one dtype")
    d = struct(**preset)
    names = {n for n, _ in struct._fields_}
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"{who}: unknown field {k}")
        setattr(d, k, v)
    return d


def _launch(who: str, d, dtype, *operands) -> None:
    name = f"dlaf_mi355x_{who}_{type_char(dtype)}"
    r = entry(name)(C.byref(d), *operands)
    if r != 0:
        raise ValueError(f"{name} refused the launch ({r})")


def update_direct(c: np.ndarray, a: np.ndarray, b: np.ndarray, *, a2: np.ndarray = None, b2: np.ndarray = None,
                  offsets=(0, 0, 0, 0, 0), repeat: bool = False, **fields):
    """ONE launch of the grouped update kernel (UpdateArgs of csrc/device/device_api.hpp) on flat host arrays.

    `c`, `a`, `b` (and `a2`, `b2` with K1 > 0) are one-dimensional arrays of the same dtype holding the operands as
    the kernel addresses them; `fields` are the fields of struct dlaf_mi355x_update_desc (strides and leading
    dimensions in elements); `offsets` are the element offsets of (c, a, b, a2, b2) into their device allocations.
    `c` is updated in place.  Returns (persistent, exclusive, c_again): how many launches took the persistent / the
    exclusive form, and with `repeat` the result of the same launch repeated on the original `c` with the counter
    words the first launch left behind (else None)."""
    ops = [c, a, b] + ([a2, b2] if fields.get("K1", 0) > 0 else [])
    d = _descriptor("update_direct", UpdateDesc, ops, fields, b_period=1, b_jl0=-1)
    d.c_elems, d.a_elems, d.b_elems = c.size, a.size, b.size
    d.a2_elems = a2.size if a2 is not None else 0
    d.b2_elems = b2.size if b2 is not None else 0
    d.c_off, d.a_off, d.b_off, d.a2_off, d.b2_off = offsets
    again = np.empty_like(c) if repeat else None
    _launch("update_direct", d, c.dtype, ptr(c), ptr(a), ptr(b), ptr(a2), ptr(b2), ptr(again))
    return int(d.persistent), int(d.exclusive), again


TRSM_PATHS = ("strips", "rows-256", "rows-128", "rows-z")
WINV_SOURCES = {"invert_diag_blocks": 0, "potrf_diag": 1, "caller": 2}


def trsm_direct(b: np.ndarray, l: np.ndarray, winv: np.ndarray, *, winv_source: str = "invert_diag_blocks",
                offsets=(0, 0, 0), **fields):
    """ONE launch of the panel TRSM (TrsmArgs of csrc/device/device_api.hpp) on flat host arrays.

    `b`, `l`, `winv` are one-dimensional arrays of the same dtype holding the operands as the kernel addresses them;
    `fields` are the fields of struct dlaf_mi355x_trsm_desc (strides and leading dimensions in elements); `offsets` are
    the element offsets of (b, l, winv) into their device allocations.  `winv_source` says who fills winv on the
    device: launch_invert_diag_blocks, a per-block loop of launch_potrf_diag(factor = false), or the caller's array.
    `b` and `winv` come back as the device left them.  Returns (path, vec, info): the kernel trsm_path chose (one of
    TRSM_PATHS), whether the strips kernel may use its 16-byte loaders, and the device info word after the launches."""
    d = _descriptor("trsm_direct", TrsmDesc, (b, l, winv), fields)
    d.winv_source = WINV_SOURCES[winv_source]
    d.b_elems, d.l_elems, d.w_elems = b.size, l.size, winv.size
    d.b_off, d.l_off, d.w_off = offsets
    _launch("trsm_direct", d, b.dtype, ptr(b), ptr(l), ptr(winv))
    return TRSM_PATHS[d.path], bool(d.vec), int(d.info_out)


POTRF_PATHS = {"coop": 0, "chain": 1}


def potrf_direct(tile: np.ndarray, winv: np.ndarray, *, path: str = "coop", offsets=(0, 0), **fields):
    """ONE factorization of one kb x kb diagonal tile (launch_potrf_coop, or the chain of launch_potrf_diag, launch_trsm
    and launch_update per 64 columns: csrc/device/device_api.hpp) on flat host arrays.

    `tile` and `winv` are one-dimensional arrays of the same dtype holding the buffers as the kernels address them;
    `fields` are the fields of struct dlaf_mi355x_potrf_desc (kb, ld, info, info_base, sync_zeroed_by, count_strips);
    `offsets` are the element offsets of (tile, winv) into their device allocations; the elements in front of each
    array hold a byte pattern on the device.  Both arrays come back as the device left them.  Returns (info, changed):
    the device info word after the launches, and the number of bytes in front of the two arrays that the launches
    changed (0 unless a kernel stored in front of a buffer)."""
    d = _descriptor("potrf_direct", PotrfDesc, (tile, winv), fields)
    d.path = POTRF_PATHS[path]
    d.t_elems, d.w_elems = tile.size, winv.size
    d.t_off, d.w_off = offsets
    _launch("potrf_direct", d, tile.dtype, ptr(tile), ptr(winv))
    return int(d.info_out), int(d.t_before_changed) + int(d.w_before_changed)
