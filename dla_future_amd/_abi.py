"""What the wrapper modules share when they cross the C ABI: pointers and leading dimensions of numpy arrays, boxed
scalars, the two descriptor forms, the global-size rule, and an entry lookup that checks the return code.  Only what at
least three wrappers use lives here; anything about one routine stays with that routine."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import DLAFDescriptor, lib


def ld_of(a: np.ndarray) -> int:
    if a.ndim != 2:
        raise ValueError("expected a 2-D array")
    if a.size and a.strides[0] != a.itemsize:
        raise ValueError("local matrices must be column-major (Fortran order)")
    return max(1, a.strides[1] // a.itemsize) if a.shape[1] > 1 else max(1, a.shape[0])


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def real_dtype(dtype):
    return np.dtype(dtype).type(0).real.dtype


def scalar(value, dtype):
    """`value` boxed as one element of `dtype`; the pointer keeps its array alive."""
    return ptr(np.array([value], dtype=dtype))


def desc9(desc):
    """The 9-int ScaLAPACK descriptor {1, ctxt, M, N, MB, NB, RSRC, CSRC, LLD} as the C array the p? entries take."""
    return (C.c_int * 9)(*[int(x) for x in desc])


def descriptor(m: int, n: int, block, src, ld: int) -> DLAFDescriptor:
    """struct DLAF_descriptor of an m x n matrix; block: nb or (mb, nb); src: the source process (row, column)."""
    mb, nb = (block, block) if np.isscalar(block) else block
    return DLAFDescriptor(m, n, mb, nb, src[0], src[1], 0, 0, ld)


def make_descriptor(n: int, nb: int, ld: int, isrc: int = 0, jsrc: int = 0) -> DLAFDescriptor:
    return descriptor(n, n, nb, (isrc, jsrc), max(1, ld))


def global_sizes(grid, given, local, subject: str):
    """`given` when all of it is; else, on a one-process grid only, `local`: the sizes of the local arrays, or a callable
    that gives them."""
    if any(x is None for x in given):
        if grid.nranks != 1:
            raise ValueError(f"{subject} required on a distributed grid")
        return local() if callable(local) else local
    return given


def global_size(grid, n, a: np.ndarray) -> int:
    return global_sizes(grid, (n,), a.shape[:1], "the global size n is")[0]


def entry(name: str):
    return getattr(lib(), name)


def check(name: str, *args) -> None:
    """Calls the entry; a return code other than 0 is a ValueError."""
    r = entry(name)(*args)
    if r != 0:
        raise ValueError(f"{name} failed with {r}")


def check_stage(name: str, *args) -> None:
    """The same for the eigensolver stages and drivers, whose failures are a RuntimeError."""
    r = entry(name)(*args)
    if r != 0:
        raise RuntimeError(f"{name} returned {r}")


def info_of(name: str, *args) -> int:
    """Calls a p? entry whose last argument is `info`; returns it."""
    info = C.c_int(-999)
    entry(name)(*args, C.byref(info))
    return info.value


def two_doubles(name: str):
    """The (ms, flops or bytes) pair of a *_profile entry."""
    a, b = C.c_double(0), C.c_double(0)
    entry(name)(C.byref(a), C.byref(b))
    return a.value, b.value
