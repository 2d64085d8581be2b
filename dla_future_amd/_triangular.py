"""The one body behind triangular_solver and triangular_multiplication (solver.py, multiplication.py): the two take the
same arguments and differ in the entry they call, as TriangularOp says on the C++ side (csrc/host/c_api_host.cpp)."""
from __future__ import annotations

from ._abi import check, desc9, descriptor, entry, global_sizes, ld_of, ptr, scalar
from .capi import type_char


def on_grid(op: str, grid, side, uplo, trans, diag, alpha, a, b, nb, m, n, a_src, b_src, b_block) -> None:
    """op: "solver" or "multiplication" (dlaf_mi355x_triangular_<op>_{s,d,c,z})."""
    t = type_char(b.dtype)
    if a.dtype != b.dtype:
        raise ValueError("A and B must have the same element type")
    m, n = global_sizes(grid, (m, n), b.shape, "the global size m x n of B is")
    na = m if side.upper() == "L" else n
    da = descriptor(na, na, nb, a_src, ld_of(a))
    db = descriptor(m, n, b_block if b_block is not None else nb, b_src, ld_of(b))
    check(f"dlaf_mi355x_triangular_{op}_{t}", grid.context, side.encode(), uplo.encode(), trans.encode(), diag.encode(),
          scalar(alpha, b.dtype), ptr(a), da, ptr(b), db)


def scalapack(routine: str, side, uplo, trans, diag, m, n, alpha, a, ia, ja, desca, b, ib, jb, descb) -> None:
    """routine: "trsm" or "trmm" (dlaf_mi355x_p{s,d,c,z}<routine>)."""
    entry(f"dlaf_mi355x_p{type_char(b.dtype)}{routine}")(side.encode(), uplo.encode(), trans.encode(), diag.encode(), m, n,
                                                        scalar(alpha, b.dtype), ptr(a), ia, ja, desc9(desca), ptr(b), ib,
                                                        jb, desc9(descb))


def resident(op: str, side, uplo, trans, diag, alpha, a, b) -> None:
    check(f"dlaf_mi355x_triangular_{op}_device", side.encode(), uplo.encode(), trans.encode(), diag.encode(),
          scalar(alpha, b.dtype), a._h, b._h)
