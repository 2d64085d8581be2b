"""dlaf_initialize / dlaf_finalize and the process grid (include/dlaf_c/init.h, include/dlaf_c/grid.h; csrc/host/grid.cpp)."""
from __future__ import annotations

import ctypes as C

from .capi import BARRIER_FN, BCAST_FN, lib


def initialize(print_config: bool = False) -> None:
    """dlaf_initialize (include/dlaf_c/init.h:27).  Idempotent."""
    args = [b"dlaf"] + ([b"--dlaf:print-config"] if print_config else [])
    argv = (C.c_char_p * len(args))(*args)
    lib().dlaf_initialize(0, None, len(args), argv)


def finalize() -> None:
    """dlaf_finalize (include/dlaf_c/init.h:35).  Idempotent; frees every grid."""
    lib().dlaf_finalize()


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
