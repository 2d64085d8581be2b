"""Host-side mirror of the reference's Cholesky interface over the C ABI.

Names and argument meaning follow the reference (file:line in the docstrings); arrays are numpy,
column-major ("F" order) like every DLA-Future local matrix.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import BARRIER_FN, BCAST_FN, DLAFDescriptor, lib, type_char


def initialize(print_config: bool = False) -> None:
    """dlaf_initialize (include/dlaf_c/init.h:27).  Idempotent."""
    args = [b"dlaf"] + ([b"--dlaf:print-config"] if print_config else [])
    argv = (C.c_char_p * len(args))(*args)
    lib().dlaf_initialize(0, None, len(args), argv)


def finalize() -> None:
    """dlaf_finalize (include/dlaf_c/init.h:35).  Idempotent; frees every grid."""
    lib().dlaf_finalize()


def make_descriptor(n: int, nb: int, ld: int, isrc: int = 0, jsrc: int = 0) -> DLAFDescriptor:
    return DLAFDescriptor(n, n, nb, nb, isrc, jsrc, 0, 0, max(1, ld))


def _ld_of(a: np.ndarray) -> int:
    if a.ndim != 2:
        raise ValueError("expected a 2-D array")
    if a.size and a.strides[0] != a.itemsize:
        raise ValueError("local matrices must be column-major (Fortran order)")
    return max(1, a.strides[1] // a.itemsize) if a.shape[1] > 1 else max(1, a.shape[0])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Grid:
    """A process grid (reference: comm::CommunicatorGrid, communication/communicator_grid.h:37-153;
    C side dlaf_create_grid, include/dlaf_c/grid.h:31).  Build one with

      Grid.single()                         1x1, no communication
      Grid.rccl(unique_id, ...)             RCCL over xGMI (production multi-GPU)
      Grid.from_torch(nprow, npcol, order)  RCCL, unique id shipped through torch.distributed
      Grid.host(..., bcast, barrier)        host-staged broadcasts supplied by the caller
    """

    def __init__(self, context: int, nranks: int, rank: int, keep=None):
        if context < 0:
            raise ValueError("grid creation failed (bad shape/rank?)")
        self.context = context
        self.nranks = nranks
        self.rank = rank
        self._keep = keep  # callbacks must outlive the grid
        r = [C.c_int() for _ in range(4)]
        lib().dlaf_mi355x_grid_info(context, *(C.byref(x) for x in r))
        self.nprow, self.npcol, self.myrow, self.mycol = (x.value for x in r)

    @classmethod
    def single(cls) -> "Grid":
        return cls(lib().dlaf_mi355x_create_grid_single(), 1, 0)

    @classmethod
    def rccl(cls, unique_id: bytes, nranks: int, rank: int, nprow: int, npcol: int, order: str = "R") -> "Grid":
        buf = C.create_string_buffer(bytes(unique_id), 128)
        ctx = lib().dlaf_mi355x_create_grid_rccl(buf, nranks, rank, nprow, npcol, order.encode())
        return cls(ctx, nranks, rank)

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        lib().dlaf_mi355x_rccl_unique_id(buf)
        return buf.raw

    @classmethod
    def from_torch(cls, nprow: int, npcol: int, order: str = "R") -> "Grid":
        """One process per GPU launched by torch.distributed.run: rank 0 makes the RCCL unique id
        and broadcasts it through the default process group."""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        if world == 1:
            return cls.single()
        box = [cls.rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls.rccl(box[0], world, rank, nprow, npcol, order)

    @classmethod
    def host(cls, nranks: int, rank: int, nprow: int, npcol: int, order: str, bcast, barrier=None) -> "Grid":
        """bcast(axis, root, memoryview) must broadcast the buffer in place along this process's
        row (axis 0, root = process column) or column (axis 1, root = process row) communicator."""

        def _bcast(_user, axis, root, buf, nbytes):
            try:
                mv = (C.c_char * nbytes).from_address(buf)
                bcast(axis, root, memoryview(mv).cast("B"))
                return 0
            except Exception as e:  # pragma: no cover - surfaced as a fatal error by the library
                print(f"[dla_future_amd] host broadcast failed: {e!r}")
                return 1

        def _barrier(_user):
            if barrier is not None:
                barrier()
            return 0

        cb, cbar = BCAST_FN(_bcast), BARRIER_FN(_barrier)
        ctx = lib().dlaf_mi355x_create_grid_host(nranks, rank, nprow, npcol, order.encode(), cb, cbar, None)
        return cls(ctx, nranks, rank, keep=(cb, cbar))

    def barrier(self) -> None:
        lib().dlaf_mi355x_grid_barrier(self.context)

    def selftest(self, nbytes: int = 1 << 20) -> int:
        """Collective wiring check of the row / column communicators; number of failed checks (0 = good)."""
        return int(lib().dlaf_mi355x_grid_selftest(self.context, nbytes))

    def comm_log(self, enable: bool = True) -> None:
        """Start (and clear) / stop the communication log of this grid (dlaf_mi355x_grid_comm_log)."""
        lib().dlaf_mi355x_grid_comm_log(self.context, 1 if enable else 0)

    def comm_log_events(self):
        """[(kind, root, bytes, grouped), ...] recorded since comm_log(True): kind 0 row broadcast, 1 column
        broadcast, 2 step marker (root = step), 3 barrier, 4 all-reduce."""
        n = lib().dlaf_mi355x_grid_comm_log_read(self.context, None, 0)
        buf = (C.c_long * (4 * max(1, n)))()
        lib().dlaf_mi355x_grid_comm_log_read(self.context, buf, n)
        return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]

    def free(self) -> None:
        """dlaf_free_grid (include/dlaf_c/grid.h:39)."""
        if self.context >= 0:
            lib().dlaf_free_grid(self.context)
            self.context = -1

    def local_shape(self, n: int, nb: int, isrc: int = 0, jsrc: int = 0):
        from . import distribution as d
        return (d.local_size(n, nb, self.nprow, self.myrow, isrc), d.local_size(n, nb, self.npcol, self.mycol, jsrc))


def cholesky_factorization(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                           n: int | None = None) -> int:
    """dlaf_cholesky_factorization_{s,d,c,z} (include/dlaf_c/factorization/cholesky.h:32-47) ==
    dlaf::cholesky_factorization(grid, uplo, matrix) (include/dlaf/factorization/cholesky.h:67-79).

    `a` is this process's local column-major part (host memory); factored in place in the `uplo`
    triangle.  Returns 0, or the LAPACK info of a non-positive-definite leading minor."""
    t = type_char(a.dtype)
    if n is None:
        if grid.nranks != 1:
            raise ValueError("the global size n is required on a distributed grid")
        n = a.shape[0]
    desc = make_descriptor(n, nb, _ld_of(a), isrc, jsrc)
    fn = getattr(lib(), f"dlaf_cholesky_factorization_{t}")
    return fn(grid.context, uplo.encode(), _ptr(a), desc)


def pxpotrf(uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_p{s,d,c,z}potrf (include/dlaf_c/factorization/cholesky.h:74-87); desca is the 9-int
    ScaLAPACK descriptor {1, ctxt, M, N, MB, NB, RSRC, CSRC, LLD}.  Returns info."""
    t = type_char(a.dtype)
    d = (C.c_int * 9)(*[int(x) for x in desca])
    info = C.c_int(-999)
    getattr(lib(), f"dlaf_p{t}potrf")(uplo.encode(), n, _ptr(a), ia, ja, d, C.byref(info))
    return info.value


def triangular_solver(grid: Grid, side: str, uplo: str, op: str, diag: str, alpha, a: np.ndarray, b: np.ndarray,
                      nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), b_src=(0, 0),
                      b_block: tuple[int, int] | None = None) -> None:
    """dlaf::triangular_solver(grid, side, uplo, op, diag, alpha, A, B)
    (include/dlaf/solver/triangular.h:41-177) == dlaf_mi355x_triangular_solver_{s,d,c,z}:
    side 'L': op(A) X = alpha B, side 'R': X op(A) = alpha B; `b` (this process's local column-major part of
    the m x n right-hand sides) is overwritten by X.  `a`: local part of the triangular matrix.
    `nb`: the square block of A; `b_block` = (MB, NB) of B when they differ (triangular.h:41-60: B's block along the
    triangular dimension must be A's, the other one is free)."""
    t = type_char(b.dtype)
    if a.dtype != b.dtype:
        raise ValueError("A and B must have the same element type")
    if m is None or n is None:
        if grid.nranks != 1:
            raise ValueError("the global size m x n of B is required on a distributed grid")
        m, n = b.shape
    na = m if side.upper() == "L" else n
    da = DLAFDescriptor(na, na, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    mb_b, nb_b = b_block if b_block is not None else (nb, nb)
    db = DLAFDescriptor(m, n, mb_b, nb_b, b_src[0], b_src[1], 0, 0, _ld_of(b))
    al = np.array([alpha], dtype=b.dtype)
    fn = getattr(lib(), f"dlaf_mi355x_triangular_solver_{t}")
    r = fn(grid.context, side.encode(), uplo.encode(), op.encode(), diag.encode(), _ptr(al), _ptr(a), da, _ptr(b), db)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_triangular_solver_{t} failed with {r}")


def triangular_multiplication(grid: Grid, side: str, uplo: str, op: str, diag: str, alpha, a: np.ndarray, b: np.ndarray,
                              nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), b_src=(0, 0),
                              b_block: tuple[int, int] | None = None) -> None:
    """dlaf::triangular_multiplication(grid, side, uplo, op, diag, alpha, A, B)
    (include/dlaf/multiplication/triangular.h) == dlaf_mi355x_triangular_multiplication_{s,d,c,z}:
    side 'L': B = alpha op(A) B, side 'R': B = alpha B op(A); `b` (this process's local column-major part of the
    m x n matrix B) is overwritten.  The other arguments are triangular_solver's."""
    t = type_char(b.dtype)
    if a.dtype != b.dtype:
        raise ValueError("A and B must have the same element type")
    if m is None or n is None:
        if grid.nranks != 1:
            raise ValueError("the global size m x n of B is required on a distributed grid")
        m, n = b.shape
    na = m if side.upper() == "L" else n
    da = DLAFDescriptor(na, na, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    mb_b, nb_b = b_block if b_block is not None else (nb, nb)
    db = DLAFDescriptor(m, n, mb_b, nb_b, b_src[0], b_src[1], 0, 0, _ld_of(b))
    al = np.array([alpha], dtype=b.dtype)
    fn = getattr(lib(), f"dlaf_mi355x_triangular_multiplication_{t}")
    r = fn(grid.context, side.encode(), uplo.encode(), op.encode(), diag.encode(), _ptr(al), _ptr(a), da, _ptr(b), db)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_triangular_multiplication_{t} failed with {r}")


def pxtrmm(side: str, uplo: str, op: str, diag: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}trmm: ScaLAPACK's p?trmm argument list (9-int descriptors)."""
    t = type_char(b.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    al = np.array([alpha], dtype=b.dtype)
    getattr(lib(), f"dlaf_mi355x_p{t}trmm")(side.encode(), uplo.encode(), op.encode(), diag.encode(), m, n, _ptr(al),
                                            _ptr(a), ia, ja, da, _ptr(b), ib, jb, db)


def hermitian_multiplication(grid: Grid, side: str, uplo: str, alpha, a: np.ndarray, b: np.ndarray, beta, c: np.ndarray,
                             nb: int, m: int | None = None, n: int | None = None, a_src=(0, 0), c_src=(0, 0),
                             c_block: tuple[int, int] | None = None) -> None:
    """dlaf::hermitian_multiplication(grid, side, uplo, alpha, A, B, beta, C) (include/dlaf/multiplication/hermitian.h)
    == dlaf_mi355x_hermitian_multiplication_{s,d,c,z}: side 'L': C = beta C + alpha A B, side 'R': C = beta C + alpha B A
    with A Hermitian (only its uplo triangle is read).  `a`, `b`, `c`: this process's local column-major parts; `c` is
    overwritten.  nb: A's square block; c_block: the MB x NB blocks of B and C (their block along A's dimension must be
    nb); c_src: the source process of B and C."""
    t = type_char(c.dtype)
    if a.dtype != c.dtype or b.dtype != c.dtype:
        raise ValueError("A, B and C must have the same element type")
    if m is None or n is None:
        if grid.nranks != 1:
            raise ValueError("the global size m x n of C is required on a distributed grid")
        m, n = c.shape
    na = m if side.upper() == "L" else n
    da = DLAFDescriptor(na, na, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    mb_c, nb_c = c_block if c_block is not None else (nb, nb)
    db = DLAFDescriptor(m, n, mb_c, nb_c, c_src[0], c_src[1], 0, 0, _ld_of(b))
    dc = DLAFDescriptor(m, n, mb_c, nb_c, c_src[0], c_src[1], 0, 0, _ld_of(c))
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    fn = getattr(lib(), f"dlaf_mi355x_hermitian_multiplication_{t}")
    r = fn(grid.context, side.encode(), uplo.encode(), _ptr(al), _ptr(a), da, _ptr(b), db, _ptr(be), _ptr(c), dc)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_hermitian_multiplication_{t} failed with {r}")


def pxhemm(side: str, uplo: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int,
           jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d}symm / p{c,z}hemm: ScaLAPACK's argument list (9-int descriptors)."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    name = f"dlaf_mi355x_p{t}{'hemm' if t in 'cz' else 'symm'}"
    getattr(lib(), name)(side.encode(), uplo.encode(), m, n, _ptr(al), _ptr(a), ia, ja, da, _ptr(b), ib, jb, db,
                         _ptr(be), _ptr(c), ic, jc, dc)


def general_multiplication(grid: Grid, opa: str, opb: str, alpha, a: np.ndarray, b: np.ndarray, beta, c: np.ndarray,
                           nb: int, m: int | None = None, n: int | None = None, k: int | None = None, a_src=(0, 0),
                           b_src=(0, 0), c_src=(0, 0)) -> None:
    """dlaf::multiplication::internal::generalMatrix(opA, opB, alpha, A, B, beta, C) (include/dlaf/multiplication/general.h)
    == dlaf_mi355x_general_multiplication_{s,d,c,z}: C = beta C + alpha op(A) op(B), op 'N', 'T' or 'C'.  `a`, `b`, `c`:
    this process's local column-major parts of the matrices as stored (A is m x k for 'N', k x m otherwise; B is k x n
    for 'N', n x k otherwise); `c` is overwritten.  nb: the square block of all three.  On a grid of more than one
    process only 'N' 'N' is built, m, n, k are required, A must start on C's process row and B on C's process column."""
    t = type_char(c.dtype)
    if a.dtype != c.dtype or b.dtype != c.dtype:
        raise ValueError("A, B and C must have the same element type")
    an, bn = opa.upper() == "N", opb.upper() == "N"
    if m is None or n is None or k is None:
        if grid.nranks != 1:
            raise ValueError("the global sizes m, n, k are required on a distributed grid")
        m, n = c.shape
        k = a.shape[1] if an else a.shape[0]
    da = DLAFDescriptor(m if an else k, k if an else m, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    db = DLAFDescriptor(k if bn else n, n if bn else k, nb, nb, b_src[0], b_src[1], 0, 0, _ld_of(b))
    dc = DLAFDescriptor(m, n, nb, nb, c_src[0], c_src[1], 0, 0, _ld_of(c))
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    fn = getattr(lib(), f"dlaf_mi355x_general_multiplication_{t}")
    r = fn(grid.context, opa.encode(), opb.encode(), _ptr(al), _ptr(a), da, _ptr(b), db, _ptr(be), _ptr(c), dc)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_general_multiplication_{t} failed with {r}")


def pxgemm(transa: str, transb: str, m: int, n: int, k: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}gemm: ScaLAPACK's argument list (9-int descriptors)."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    getattr(lib(), f"dlaf_mi355x_p{t}gemm")(transa.encode(), transb.encode(), m, n, k, _ptr(al), _ptr(a), ia, ja, da,
                                            _ptr(b), ib, jb, db, _ptr(be), _ptr(c), ic, jc, dc)


def _real_dtype(dtype):
    return np.dtype(dtype).type(0).real.dtype


def _rank_update(two: bool, grid: Grid, uplo: str, trans: str, alpha, a: np.ndarray, b, beta, c: np.ndarray, nb: int,
                 n, k, a_src, c_src) -> None:
    t = type_char(c.dtype)
    if a.dtype != c.dtype or (two and b.dtype != c.dtype):
        raise ValueError("the operands must have the same element type")
    tn = trans.upper() == "N"
    if n is None or k is None:
        if grid.nranks != 1:
            raise ValueError("the global sizes n, k are required on a distributed grid")
        n = c.shape[0]
        k = a.shape[1] if tn else a.shape[0]
    rdt = _real_dtype(c.dtype)
    da = DLAFDescriptor(n if tn else k, k if tn else n, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    dc = DLAFDescriptor(n, n, nb, nb, c_src[0], c_src[1], 0, 0, _ld_of(c))
    be = np.array([beta], dtype=rdt)
    if two:
        db = DLAFDescriptor(n if tn else k, k if tn else n, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(b))
        al = np.array([alpha], dtype=c.dtype)
        name = f"dlaf_mi355x_hermitian_rank_2k_update_{t}"
        r = getattr(lib(), name)(grid.context, uplo.encode(), trans.encode(), _ptr(al), _ptr(a), da, _ptr(b), db, _ptr(be),
                                 _ptr(c), dc)
    else:
        al = np.array([alpha], dtype=rdt)
        name = f"dlaf_mi355x_hermitian_rank_k_update_{t}"
        r = getattr(lib(), name)(grid.context, uplo.encode(), trans.encode(), _ptr(al), _ptr(a), da, _ptr(be), _ptr(c), dc)
    if r != 0:
        raise ValueError(f"{name} failed with {r}")


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
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al = np.array([alpha], dtype=_real_dtype(c.dtype))
    be = np.array([beta], dtype=_real_dtype(c.dtype))
    name = f"dlaf_mi355x_p{t}{'herk' if t in 'cz' else 'syrk'}"
    getattr(lib(), name)(uplo.encode(), trans.encode(), n, k, _ptr(al), _ptr(a), ia, ja, da, _ptr(be), _ptr(c), ic, jc, dc)


def pxher2k(uplo: str, trans: str, n: int, k: int, alpha, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int,
            jb: int, descb, beta, c: np.ndarray, ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d}syr2k / p{c,z}her2k: ScaLAPACK's argument list (9-int descriptors; beta real)."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=_real_dtype(c.dtype))
    name = f"dlaf_mi355x_p{t}{'her2k' if t in 'cz' else 'syr2k'}"
    getattr(lib(), name)(uplo.encode(), trans.encode(), n, k, _ptr(al), _ptr(a), ia, ja, da, _ptr(b), ib, jb, db, _ptr(be),
                         _ptr(c), ic, jc, dc)


def general_addition(grid: Grid, uplo: str, op: str, alpha, a: np.ndarray, beta, c: np.ndarray, nb: int,
                     m: int | None = None, n: int | None = None, a_src=(0, 0), c_src=(0, 0)) -> None:
    """C = beta C + alpha op(A) on the uplo part of the m x n matrix C == dlaf_mi355x_general_addition_{s,d,c,z} (PBLAS
    p?geadd / p?tradd, p?tran / p?tranu / p?tranc; ScaLAPACK p?lacpy is alpha 1, beta 0, op 'N').  uplo 'A' all, 'L' i >= j,
    'U' i <= j; op 'N' (A stored m x n), 'T' or 'C' (A stored n x m).  `a`, `c`: this process's local column-major parts;
    outside the uplo part `c` stays bit for bit; alpha 1, beta 0 with op 'N' / 'T' is a bit copy.  nb: the square block of
    both.  Any grid (m and n are required on more than one process); op 'N' needs A on C's source process, and only op
    'N' accepts `a is c`."""
    t = type_char(c.dtype)
    if a.dtype != c.dtype:
        raise ValueError("A and C must have the same element type")
    if m is None or n is None:
        if grid.nranks != 1:
            raise ValueError("the global sizes m, n are required on a distributed grid")
        m, n = c.shape
    tn = op.upper() == "N"
    da = DLAFDescriptor(m if tn else n, n if tn else m, nb, nb, a_src[0], a_src[1], 0, 0, _ld_of(a))
    dc = DLAFDescriptor(m, n, nb, nb, c_src[0], c_src[1], 0, 0, _ld_of(c))
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    name = f"dlaf_mi355x_general_addition_{t}"
    r = getattr(lib(), name)(grid.context, uplo.encode(), op.encode(), _ptr(al), _ptr(a), da, _ptr(be), _ptr(c), dc)
    if r != 0:
        raise ValueError(f"{name} failed with {r}")


def hermitian_complete(grid: Grid, uplo: str, kind: str, a: np.ndarray, nb: int, n: int | None = None, src=(0, 0)) -> None:
    """Fills the OTHER triangle of the n x n matrix from its uplo one, in place == dlaf_mi355x_hermitian_complete_{s,d,c,z}:
    kind 'H' conjugates the mirror and makes the diagonal's imaginary parts exactly 0, kind 'S' transposes plainly and
    leaves the diagonal untouched.  `a`: this process's local column-major part; nb: its square block."""
    t = type_char(a.dtype)
    if n is None:
        if grid.nranks != 1:
            raise ValueError("the global size n is required on a distributed grid")
        n = a.shape[0]
    da = DLAFDescriptor(n, n, nb, nb, src[0], src[1], 0, 0, _ld_of(a))
    name = f"dlaf_mi355x_hermitian_complete_{t}"
    r = getattr(lib(), name)(grid.context, uplo.encode(), kind.encode(), _ptr(a), da)
    if r != 0:
        raise ValueError(f"{name} failed with {r}")


def pxgeadd(trans: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray, ic: int,
            jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}geadd: PBLAS's argument list (9-int descriptors): C = beta C + alpha op(A)."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al, be = np.array([alpha], dtype=c.dtype), np.array([beta], dtype=c.dtype)
    getattr(lib(), f"dlaf_mi355x_p{t}geadd")(trans.encode(), m, n, _ptr(al), _ptr(a), ia, ja, da, _ptr(be), _ptr(c), ic, jc,
                                             dc)


def pxtradd(uplo: str, trans: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray,
            ic: int, jc: int, descc) -> None:
    """dlaf_mi355x_p{s,d,c,z}tradd: the same on the uplo ('L' / 'U') trapezoid of C."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al, be = np.array([alpha], dtype=c.dtype), np.array([beta], dtype=c.dtype)
    getattr(lib(), f"dlaf_mi355x_p{t}tradd")(uplo.encode(), trans.encode(), m, n, _ptr(al), _ptr(a), ia, ja, da, _ptr(be),
                                             _ptr(c), ic, jc, dc)


def pxtran(m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca, beta, c: np.ndarray, ic: int, jc: int, descc,
           conj: bool = False) -> None:
    """dlaf_mi355x_p{s,d}tran / p{c,z}tranu (conj False) / p{c,z}tranc (conj True): C (m x n) = beta C + alpha A^T / A^H,
    A stored n x m."""
    t = type_char(c.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    dc = (C.c_int * 9)(*[int(x) for x in descc])
    al, be = np.array([alpha], dtype=c.dtype), np.array([beta], dtype=c.dtype)
    name = f"dlaf_mi355x_p{t}tran" + (("c" if conj else "u") if t in "cz" else "")
    getattr(lib(), name)(m, n, _ptr(al), _ptr(a), ia, ja, da, _ptr(be), _ptr(c), ic, jc, dc)


def pxlacpy(uplo: str, m: int, n: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}lacpy: B = A on the uplo part; as in LAPACK any letter other than 'U' / 'L' means all."""
    t = type_char(b.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    getattr(lib(), f"dlaf_mi355x_p{t}lacpy")(uplo.encode(), m, n, _ptr(a), ia, ja, da, _ptr(b), ib, jb, db)


def addition_profile():
    """(ms, bytes) of the last general_addition / hermitian_complete / conversion on this process: device time, and the
    whole-grid algorithmic bytes (read A + write C, + read C when beta != 0; a completion reads and writes half)."""
    ms, by = C.c_double(0), C.c_double(0)
    lib().dlaf_mi355x_addition_profile(C.byref(ms), C.byref(by))
    return ms.value, by.value


def multiplication_profile():
    """(ms, flops) of the sweep of the last multiplication (triangular, Hermitian, general or Hermitian rank update) on this
    process (device time, no staging)."""
    ms, fl = C.c_double(0), C.c_double(0)
    lib().dlaf_mi355x_multiplication_profile(C.byref(ms), C.byref(fl))
    return ms.value, fl.value


def pxpotrs(uplo: str, n: int, nrhs: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb) -> int:
    """dlaf_mi355x_p{s,d,c,z}potrs: A X = B with the factor p?potrf left in `a`; returns info."""
    t = type_char(b.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    info = C.c_int(-999)
    getattr(lib(), f"dlaf_mi355x_p{t}potrs")(uplo.encode(), n, nrhs, _ptr(a), ia, ja, da, _ptr(b), ib, jb, db,
                                             C.byref(info))
    return info.value


def generalized_to_standard(grid: Grid, uplo: str, a: np.ndarray, b: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                            n: int | None = None) -> int:
    """dlaf::eigensolver::internal::generalized_to_standard(grid, uplo, mat_a, mat_b)
    (include/dlaf/eigensolver/gen_to_std.h:50, :101) == dlaf_mi355x_generalized_to_standard_{s,d,c,z}:
    `a` (this process's local part of the Hermitian A) is overwritten by inv(L) A inv(L^H) (uplo 'L') or
    inv(U^H) A inv(U) (uplo 'U') in its uplo triangle; `b` holds the Cholesky factor of B in the same triangle."""
    t = type_char(a.dtype)
    if a.dtype != b.dtype:
        raise ValueError("A and B must have the same element type")
    if n is None:
        if grid.nranks != 1:
            raise ValueError("the global size n is required on a distributed grid")
        n = a.shape[0]
    da = make_descriptor(n, nb, _ld_of(a), isrc, jsrc)
    db = make_descriptor(n, nb, _ld_of(b), isrc, jsrc)
    return getattr(lib(), f"dlaf_mi355x_generalized_to_standard_{t}")(grid.context, uplo.encode(), _ptr(a), da, _ptr(b), db)


def pxhegst(ibtype: int, uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca, b: np.ndarray, ib: int, jb: int,
            descb):
    """dlaf_mi355x_p{s,d,c,z}hegst: ScaLAPACK's p?sygst / p?hegst argument list; returns (scale, info)."""
    t = type_char(a.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    scale = (C.c_float if t in "sc" else C.c_double)(-1)
    info = C.c_int(-999)
    getattr(lib(), f"dlaf_mi355x_p{t}hegst")(ibtype, uplo.encode(), n, _ptr(a), ia, ja, da, _ptr(b), ib, jb, db,
                                             C.byref(scale), C.byref(info))
    return scale.value, info.value


def triangular_inverse(grid: Grid, uplo: str, diag: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                       n: int | None = None) -> int:
    """dlaf::triangular_inverse == dlaf_mi355x_triangular_inverse_{s,d,c,z} (LAPACK xTRTRI): the triangular matrix in the
    uplo triangle of `a` (this process's local part; diag 'N' / 'U') is overwritten by its inverse.  Returns LAPACK's
    info: i > 0 when the i-th diagonal element is exactly zero, and `a` is then untouched."""
    t = type_char(a.dtype)
    if n is None:
        if grid.nranks != 1:
            raise ValueError("the global size n is required on a distributed grid")
        n = a.shape[0]
    da = make_descriptor(n, nb, _ld_of(a), isrc, jsrc)
    return getattr(lib(), f"dlaf_mi355x_triangular_inverse_{t}")(grid.context, uplo.encode(), diag.encode(), _ptr(a), da)


def inverse_from_cholesky_factor(grid: Grid, uplo: str, a: np.ndarray, nb: int, isrc: int = 0, jsrc: int = 0,
                                 n: int | None = None) -> int:
    """dlaf::inverse_from_cholesky_factor == dlaf_mi355x_inverse_from_cholesky_factor_{s,d,c,z} (LAPACK xPOTRI): the
    uplo triangle of `a` holds the Cholesky factor and is overwritten by the same triangle of inv(L L^H) / inv(U^H U).
    Returns LAPACK's info."""
    t = type_char(a.dtype)
    if n is None:
        if grid.nranks != 1:
            raise ValueError("the global size n is required on a distributed grid")
        n = a.shape[0]
    da = make_descriptor(n, nb, _ld_of(a), isrc, jsrc)
    return getattr(lib(), f"dlaf_mi355x_inverse_from_cholesky_factor_{t}")(grid.context, uplo.encode(), _ptr(a), da)


def pxtrtri(uplo: str, diag: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_mi355x_p{s,d,c,z}trtri: ScaLAPACK's p?trtri argument list; returns info."""
    t = type_char(a.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    info = C.c_int(-999)
    getattr(lib(), f"dlaf_mi355x_p{t}trtri")(uplo.encode(), diag.encode(), n, _ptr(a), ia, ja, da, C.byref(info))
    return info.value


def pxpotri(uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> int:
    """dlaf_mi355x_p{s,d,c,z}potri: ScaLAPACK's p?potri argument list; returns info."""
    t = type_char(a.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    info = C.c_int(-999)
    getattr(lib(), f"dlaf_mi355x_p{t}potri")(uplo.encode(), n, _ptr(a), ia, ja, da, C.byref(info))
    return info.value


def inverse_profile():
    """(ms, flops) of the last triangular_inverse / inverse_from_cholesky_factor on this process (device time, no
    staging; n^3 / 3 flops per half, x 4 for complex types)."""
    ms, fl = C.c_double(0), C.c_double(0)
    lib().dlaf_mi355x_inverse_profile(C.byref(ms), C.byref(fl))
    return ms.value, fl.value


def solver_profile():
    """(ms, flops) of the sweep of the last triangular solve on this process (device time, no staging)."""
    ms, fl = C.c_double(0), C.c_double(0)
    lib().dlaf_mi355x_solver_profile(C.byref(ms), C.byref(fl))
    return ms.value, fl.value


def pxtrsm(side: str, uplo: str, op: str, diag: str, m: int, n: int, alpha, a: np.ndarray, ia: int, ja: int, desca,
           b: np.ndarray, ib: int, jb: int, descb) -> None:
    """dlaf_mi355x_p{s,d,c,z}trsm: ScaLAPACK's p?trsm argument list (9-int descriptors)."""
    t = type_char(b.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    db = (C.c_int * 9)(*[int(x) for x in descb])
    al = np.array([alpha], dtype=b.dtype)
    getattr(lib(), f"dlaf_mi355x_p{t}trsm")(side.encode(), uplo.encode(), op.encode(), diag.encode(), m, n, _ptr(al),
                                            _ptr(a), ia, ja, da, _ptr(b), ib, jb, db)


def set_random_hermitian_positive_definite(grid: Grid, a: np.ndarray, n: int, nb: int, isrc: int = 0,
                                           jsrc: int = 0, nthreads: int = 0) -> None:
    """matrix::util::set_random_hermitian_positive_definite (include/dlaf/util_matrix.h:498-501) on
    this process's local array."""
    desc = make_descriptor(n, nb, _ld_of(a), isrc, jsrc)
    r = lib().dlaf_mi355x_set_random_hpd(grid.context, type_char(a.dtype).encode(), _ptr(a), desc, nthreads)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_set_random_hpd failed with {r}")


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


class DeviceMatrix:
    """Matrix<T, Device::GPU> of the MI355X build: the local part of a block-cyclic matrix resident
    in HBM in tile layout (reference: matrix/matrix.h:57-357 + MatrixMirror, matrix_mirror.h:137-173).
    A driver uploads once and times `factorize` alone, like miniapp_cholesky.cpp:133-155."""

    def __init__(self, grid: Grid, dtype, uplo: str, n: int, nb: int, isrc: int = 0, jsrc: int = 0):
        self.grid, self.dtype, self.uplo, self.n, self.nb = grid, np.dtype(dtype), uplo, n, nb
        self._h = C.c_void_p()
        desc = make_descriptor(n, nb, 1, isrc, jsrc)
        r = lib().dlaf_mi355x_matrix_create(grid.context, type_char(dtype).encode(), uplo.encode(), desc,
                                            C.byref(self._h))
        if r != 0:
            raise ValueError(f"dlaf_mi355x_matrix_create failed with {r}")

    def upload(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_matrix_upload(self._h, _ptr(a), _ld_of(a))

    def download(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_matrix_download(self._h, _ptr(a), _ld_of(a))

    def fetch_tile(self, gi: int, gj: int):
        """Global tile (gi, gj) of the device copy as a dense column-major array, or None when this process
        does not own it (a checker samples a large factor tile by tile instead of downloading it whole)."""
        rows = min(self.nb, self.n - gi * self.nb)
        cols = min(self.nb, self.n - gj * self.nb)
        out = np.zeros((rows, cols), dtype=self.dtype, order="F")
        r = lib().dlaf_mi355x_matrix_fetch_tile(self._h, gi, gj, _ptr(out), max(1, rows))
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
        r = lib().dlaf_mi355x_matrix_to_general(kind.encode(), self._h, g._h)
        if r != 0:
            raise ValueError(f"dlaf_mi355x_matrix_to_general failed with {r}")

    def from_general(self, g: "GeneralDeviceMatrix") -> None:
        """Takes this matrix's uplo triangle from the resident general matrix `g`; nothing crosses PCIe."""
        r = lib().dlaf_mi355x_matrix_from_general(self._h, g._h)
        if r != 0:
            raise ValueError(f"dlaf_mi355x_matrix_from_general failed with {r}")

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
        desc = DLAFDescriptor(m, n, nb, nb, isrc, jsrc, 0, 0, 1)
        r = lib().dlaf_mi355x_gmatrix_create(grid.context, type_char(dtype).encode(), desc, C.byref(self._h))
        if r != 0:
            raise ValueError(f"dlaf_mi355x_gmatrix_create failed with {r}")

    def upload(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_gmatrix_upload(self._h, _ptr(a), _ld_of(a))

    def download(self, a: np.ndarray) -> None:
        assert a.dtype == self.dtype
        lib().dlaf_mi355x_gmatrix_download(self._h, _ptr(a), _ld_of(a))

    def close(self) -> None:
        if self._h:
            lib().dlaf_mi355x_gmatrix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def triangular_solver_device(side: str, uplo: str, op: str, diag: str, alpha, a: DeviceMatrix, b: GeneralDeviceMatrix) -> None:
    """dlaf::triangular_solver on resident operands: `a` holds the triangular matrix in its uplo triangle (e.g. the
    factor a.factorize() left there), `b` is overwritten by the solution; no PCIe traffic."""
    al = np.array([alpha], dtype=b.dtype)
    r = lib().dlaf_mi355x_triangular_solver_device(side.encode(), uplo.encode(), op.encode(), diag.encode(), _ptr(al),
                                                   a._h, b._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_triangular_solver_device failed with {r}")


def triangular_multiplication_device(side: str, uplo: str, op: str, diag: str, alpha, a: DeviceMatrix,
                                     b: GeneralDeviceMatrix) -> None:
    """dlaf::triangular_multiplication on resident operands: `a` holds the triangular matrix in its uplo triangle
    (e.g. the factor a.factorize() left there), `b` is overwritten by the product; no PCIe traffic."""
    al = np.array([alpha], dtype=b.dtype)
    r = lib().dlaf_mi355x_triangular_multiplication_device(side.encode(), uplo.encode(), op.encode(), diag.encode(),
                                                           _ptr(al), a._h, b._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_triangular_multiplication_device failed with {r}")


def hermitian_multiplication_device(side: str, uplo: str, alpha, a: DeviceMatrix, b: GeneralDeviceMatrix, beta,
                                    c: GeneralDeviceMatrix) -> None:
    """dlaf::hermitian_multiplication on resident operands: `a` holds the Hermitian matrix in its uplo triangle, `b` and
    `c` are general resident matrices of the same shape; only `c` is written; no PCIe traffic."""
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    r = lib().dlaf_mi355x_hermitian_multiplication_device(side.encode(), uplo.encode(), _ptr(al), a._h, b._h, _ptr(be),
                                                          c._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_hermitian_multiplication_device failed with {r}")


def general_multiplication_device(opa: str, opb: str, alpha, a: GeneralDeviceMatrix, b: GeneralDeviceMatrix, beta,
                                  c: GeneralDeviceMatrix) -> None:
    """general_multiplication on resident operands: C = beta C + alpha op(A) op(B) on three general resident matrices
    (`a`, `b` as stored); only `c` is written; no PCIe traffic."""
    al = np.array([alpha], dtype=c.dtype)
    be = np.array([beta], dtype=c.dtype)
    r = lib().dlaf_mi355x_general_multiplication_device(opa.encode(), opb.encode(), _ptr(al), a._h, b._h, _ptr(be), c._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_general_multiplication_device failed with {r}")


def hermitian_rank_k_update_device(uplo: str, trans: str, alpha, a: GeneralDeviceMatrix, beta, c: DeviceMatrix) -> None:
    """hermitian_rank_k_update on resident operands: `c` a DeviceMatrix created with this uplo (what factorize() takes),
    `a` a general resident matrix as stored; only the uplo triangle of `c` is written; no PCIe traffic."""
    rdt = _real_dtype(a.dtype)
    al, be = np.array([alpha], dtype=rdt), np.array([beta], dtype=rdt)
    r = lib().dlaf_mi355x_hermitian_rank_k_update_device(uplo.encode(), trans.encode(), _ptr(al), a._h, _ptr(be), c._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_hermitian_rank_k_update_device failed with {r}")


def hermitian_rank_2k_update_device(uplo: str, trans: str, alpha, a: GeneralDeviceMatrix, b: GeneralDeviceMatrix, beta,
                                    c: DeviceMatrix) -> None:
    """hermitian_rank_2k_update on resident operands (`a`, `b` general resident matrices as stored, `c` a DeviceMatrix
    created with this uplo); only the uplo triangle of `c` is written; no PCIe traffic."""
    al = np.array([alpha], dtype=a.dtype)
    be = np.array([beta], dtype=_real_dtype(a.dtype))
    r = lib().dlaf_mi355x_hermitian_rank_2k_update_device(uplo.encode(), trans.encode(), _ptr(al), a._h, b._h, _ptr(be),
                                                          c._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_hermitian_rank_2k_update_device failed with {r}")


def general_addition_device(uplo: str, op: str, alpha, a: GeneralDeviceMatrix, beta, c: GeneralDeviceMatrix) -> None:
    """general_addition on resident general matrices (`a` as stored; only the uplo part of `c` is written; `a is c` is op
    'N' in place); no PCIe traffic."""
    al, be = np.array([alpha], dtype=c.dtype), np.array([beta], dtype=c.dtype)
    r = lib().dlaf_mi355x_general_addition_device(uplo.encode(), op.encode(), _ptr(al), a._h, _ptr(be), c._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_general_addition_device failed with {r}")


def hermitian_complete_device(uplo: str, kind: str, a: GeneralDeviceMatrix) -> None:
    """hermitian_complete on a resident general matrix, in place; no PCIe traffic."""
    r = lib().dlaf_mi355x_hermitian_complete_device(uplo.encode(), kind.encode(), a._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_hermitian_complete_device failed with {r}")


def potrs_device(uplo: str, factor: DeviceMatrix, b: GeneralDeviceMatrix) -> None:
    """A X = B from the resident Cholesky factor (the two solves of p?potrs, all in HBM)."""
    r = lib().dlaf_mi355x_potrs_device(uplo.encode(), factor._h, b._h)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_potrs_device failed with {r}")


NORM_ERRORS = {-1: "bad norm letter", -2: "bad uplo", -3: "bad diag", -4: "bad descriptor", -5: "source process outside the grid",
               -6: "missing value or context"}


def matrix_norm(grid: Grid, norm: str, a: np.ndarray, nb: int, structure: str = "G", uplo: str = "L", diag: str = "N",
                m: int | None = None, n: int | None = None, isrc: int = 0, jsrc: int = 0) -> float:
    """dlaf::auxiliary::max_norm and its one / infinity / Frobenius siblings == dlaf_mi355x_{general,hermitian,
    triangular}_norm_{s,d,c,z} (LAPACK xLANGE, xLANHE / xLANSY, xLANTR).  norm: 'M', '1' / 'O', 'I', 'F' / 'E';
    structure 'G' (the m x n matrix), 'H' (Hermitian from the uplo triangle) or 'T' (triangular, diag 'N' / 'U').
    `a`: this process's local column-major part, only read.  The value is the same on every rank."""
    t = type_char(a.dtype)
    if m is None or n is None:
        if grid.nranks != 1:
            raise ValueError("the global size m x n is required on a distributed grid")
        m, n = a.shape
    da = DLAFDescriptor(m, n, nb, nb, isrc, jsrc, 0, 0, _ld_of(a))
    v = C.c_double(-1.0)
    s = structure.upper()
    if s == "G":
        r = getattr(lib(), f"dlaf_mi355x_general_norm_{t}")(grid.context, norm.encode(), _ptr(a), da, C.byref(v))
    elif s in ("H", "S"):
        r = getattr(lib(), f"dlaf_mi355x_hermitian_norm_{t}")(grid.context, norm.encode(), uplo.encode(), _ptr(a), da,
                                                              C.byref(v))
    elif s == "T":
        r = getattr(lib(), f"dlaf_mi355x_triangular_norm_{t}")(grid.context, norm.encode(), uplo.encode(), diag.encode(),
                                                               _ptr(a), da, C.byref(v))
    else:
        raise ValueError(f"structure must be 'G', 'H' or 'T', got {structure!r}")
    if r != 0:
        raise ValueError(f"matrix_norm failed with {r}: {NORM_ERRORS.get(r, '?')}")
    return v.value


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
    if r != 0:
        raise ValueError(f"matrix_norm_device failed with {r}: {NORM_ERRORS.get(r, '?')}")
    return v.value


def pxlange(norm: str, m: int, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{s,d,c,z}lange: ScaLAPACK's p?lange argument list without work; returns the value."""
    da = (C.c_int * 9)(*[int(x) for x in desca])
    return float(getattr(lib(), f"dlaf_mi355x_p{type_char(a.dtype)}lange")(norm.encode(), m, n, _ptr(a), ia, ja, da))


def pxlanhe(norm: str, uplo: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{c,z}lanhe / p{s,d}lansy: ScaLAPACK's argument list without work; returns the value."""
    t = type_char(a.dtype)
    da = (C.c_int * 9)(*[int(x) for x in desca])
    name = f"dlaf_mi355x_p{t}lan{'he' if t in 'cz' else 'sy'}"
    return float(getattr(lib(), name)(norm.encode(), uplo.encode(), n, _ptr(a), ia, ja, da))


def pxlantr(norm: str, uplo: str, diag: str, n: int, a: np.ndarray, ia: int, ja: int, desca) -> float:
    """dlaf_mi355x_p{s,d,c,z}lantr: ScaLAPACK's p?lantr argument list without work; returns the value."""
    da = (C.c_int * 9)(*[int(x) for x in desca])
    return float(getattr(lib(), f"dlaf_mi355x_p{type_char(a.dtype)}lantr")(norm.encode(), uplo.encode(), diag.encode(), n,
                                                                         _ptr(a), ia, ja, da))


def norm_profile():
    """(ms, bytes) of the last norm on this process: device time (no upload) and the bytes of the tiles it referenced
    (diagonal tiles counted whole)."""
    ms, by = C.c_double(0), C.c_double(0)
    lib().dlaf_mi355x_norm_profile(C.byref(ms), C.byref(by))
    return ms.value, by.value


# ---- tile operations with the argument sets the factorization issues ----------------------------
def tile_potrf(uplo: str, a: np.ndarray) -> int:
    """tile::potrf (include/dlaf/lapack/tile.h:362-378); returns info."""
    return lib().dlaf_mi355x_tile_potrf(type_char(a.dtype).encode(), uplo.encode(), a.shape[0], _ptr(a), _ld_of(a))


def tile_trsm(uplo: str, a: np.ndarray, b: np.ndarray) -> None:
    """tile::trsm as cholesky/impl.h:56-67 (L: B <- B A^-H) / :110-121 (U: B <- A^-H B) call it."""
    m, n = b.shape
    lib().dlaf_mi355x_tile_trsm(type_char(b.dtype).encode(), uplo.encode(), m, n, _ptr(a), _ld_of(a), _ptr(b),
                                _ld_of(b))


def tile_herk(uplo: str, a: np.ndarray, c: np.ndarray) -> None:
    """tile::herk as impl.h:70-80 (L: C -= A A^H) / :124-134 (U: C -= A^H A) call it."""
    n = c.shape[0]
    k = a.shape[1] if uplo in "Ll" else a.shape[0]
    lib().dlaf_mi355x_tile_herk(type_char(c.dtype).encode(), uplo.encode(), n, k, _ptr(a), _ld_of(a), _ptr(c),
                                _ld_of(c))


def tile_gemm(uplo: str, a: np.ndarray, b: np.ndarray, c: np.ndarray) -> None:
    """tile::gemm as impl.h:83-94 (L: C -= A B^H) / :137-147 (U: C -= A^H B) call it."""
    m, n = c.shape
    k = a.shape[1] if uplo in "Ll" else a.shape[0]
    lib().dlaf_mi355x_tile_gemm(type_char(c.dtype).encode(), uplo.encode(), m, n, k, _ptr(a), _ld_of(a), _ptr(b),
                                _ld_of(b), _ptr(c), _ld_of(c))


def update_bulk_slots(dtype) -> int:
    """Workgroup slots of the bulk update kernel on this GPU for `dtype` (what the drivers size persistent launches by)."""
    return int(lib().dlaf_mi355x_update_bulk_slots(type_char(dtype).encode()))


def update_direct(c: np.ndarray, a: np.ndarray, b: np.ndarray, *, a2: np.ndarray = None, b2: np.ndarray = None,
                  offsets=(0, 0, 0, 0, 0), repeat: bool = False, **fields):
    """ONE launch of the grouped update kernel (UpdateArgs of csrc/device/device_api.hpp) on flat host arrays.

    `c`, `a`, `b` (and `a2`, `b2` with K1 > 0) are one-dimensional arrays of the same dtype holding the operands as
    the kernel addresses them; `fields` are the fields of struct dlaf_mi355x_update_desc (strides and leading
    dimensions in elements); `offsets` are the element offsets of (c, a, b, a2, b2) into their device allocations.
    `c` is updated in place.  Returns (persistent, exclusive, c_again): how many launches took the persistent / the
    exclusive form, and with `repeat` the result of the same launch repeated on the original `c` with the counter
    words the first launch left behind (else None)."""
    from .capi import UpdateDesc
    ops = [c, a, b] + ([a2, b2] if fields.get("K1", 0) > 0 else [])
    for x in ops:
        if x is None or x.ndim != 1 or x.dtype != c.dtype or not x.flags.c_contiguous:
            raise ValueError("update_direct takes flat contiguous arrays of one dtype")
    d = UpdateDesc()
    d.b_period, d.b_jl0 = 1, -1
    for k, v in fields.items():
        if k not in {n for n, _ in UpdateDesc._fields_}:
            raise TypeError(f"update_direct: unknown field {k}")
        setattr(d, k, v)
    d.c_elems, d.a_elems, d.b_elems = c.size, a.size, b.size
    d.a2_elems = a2.size if a2 is not None else 0
    d.b2_elems = b2.size if b2 is not None else 0
    d.c_off, d.a_off, d.b_off, d.a2_off, d.b2_off = offsets
    again = np.empty_like(c) if repeat else None
    fn = getattr(lib(), "dlaf_mi355x_update_direct_" + type_char(c.dtype))
    r = fn(C.byref(d), _ptr(c), _ptr(a), _ptr(b), _ptr(a2) if a2 is not None else None,
           _ptr(b2) if b2 is not None else None, _ptr(again) if repeat else None)
    if r != 0:
        raise ValueError(f"dlaf_mi355x_update_direct_{type_char(c.dtype)} refused the launch ({r})")
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
    from .capi import TrsmDesc
    for x in (b, l, winv):
        if x is None or x.ndim != 1 or x.dtype != b.dtype or not x.flags.c_contiguous:
            raise ValueError("trsm_direct takes flat contiguous arrays of one dtype")
    d = TrsmDesc()
    names = {n for n, _ in TrsmDesc._fields_}
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"trsm_direct: unknown field {k}")
        setattr(d, k, v)
    d.winv_source = WINV_SOURCES[winv_source]
    d.b_elems, d.l_elems, d.w_elems = b.size, l.size, winv.size
    d.b_off, d.l_off, d.w_off = offsets
    fn = getattr(lib(), "dlaf_mi355x_trsm_direct_" + type_char(b.dtype))
    r = fn(C.byref(d), _ptr(b), _ptr(l), _ptr(winv))
    if r != 0:
        raise ValueError(f"dlaf_mi355x_trsm_direct_{type_char(b.dtype)} refused the launch ({r})")
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
    from .capi import PotrfDesc
    for x in (tile, winv):
        if x is None or x.ndim != 1 or x.dtype != tile.dtype or not x.flags.c_contiguous:
            raise ValueError("potrf_direct takes flat contiguous arrays of one dtype")
    d = PotrfDesc()
    names = {n for n, _ in PotrfDesc._fields_}
    for k, v in fields.items():
        if k not in names:
            raise TypeError(f"potrf_direct: unknown field {k}")
        setattr(d, k, v)
    d.path = POTRF_PATHS[path]
    d.t_elems, d.w_elems = tile.size, winv.size
    d.t_off, d.w_off = offsets
    fn = getattr(lib(), "dlaf_mi355x_potrf_direct_" + type_char(tile.dtype))
    r = fn(C.byref(d), _ptr(tile), _ptr(winv))
    if r != 0:
        raise ValueError(f"dlaf_mi355x_potrf_direct_{type_char(tile.dtype)} refused the launch ({r})")
    return int(d.info_out), int(d.t_before_changed) + int(d.w_before_changed)
