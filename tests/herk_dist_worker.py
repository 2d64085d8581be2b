"""Worker of the distributed Hermitian rank-k / rank-2k update test (tests/test_gpu_hermitian_rank_update_grid.py): one
process per rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of
dist_worker.py).  Trans N (the SUMMA sweep with the transposed-panel broadcast) on exact operands -- integer entries in
[-3, 3], n = 5 nb + 3 at nb = 32 (on 2 x 3 the transposed panel has more than one class per root row and a ragged last
tile row), k = 72 (three k tiles) -- for d and z, both updates, both uplo, zero and non-zero source processes, and once
more per type and update (uplo U, the non-zero sources) with k = 200: 2 kBuf + 1 = 7 k tiles with a ragged last one, so
that the sweep's ring of kBuf = 3 operand buffers is reused twice and the wait that guards the reuse runs (the sums stay
below 2 * 4 * 9 * 200, exact in fp64) -- through the host entry and the resident one; every rank compares its local part
of the triangle with equality and its part of the other triangle, filled with NaN, bit for bit, and checks that its parts
of A and B did not change."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    nprow, npcol, order = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo")
    import dla_future_amd as dlaf
    from oracle import oracle
    from dist_worker import make_grid
    from test_gpu_hermitian_rank_update import DT, in_triangle, integers, operands, reference, scalars

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    me = (grid.myrow, grid.mycol)

    def said(cond, what):
        """a check that would otherwise fail without a word: say which one (every rank, once)"""
        if not cond:
            print(f"[herk_dist_worker] rank {rank} {me}: FAILED {what}", flush=True)
        return bool(cond)

    ok = True
    nb = 32
    n = 5 * nb + 3
    r1, c1 = nprow - 1, npcol - 1
    # (source of C, column source of A and B): A starts on C's process row; its columns elsewhere where there is room
    sources = [((0, 0), 0), ((r1, c1), c1 - 1 if npcol > 2 else c1)]
    for t in ("d", "z"):
        dt = DT[t]
        for two in (False, True):
            alpha, beta = scalars(t, two)
            for uplo, k, srcs in (("L", 72, sources), ("U", 72, sources), ("U", 6 * nb + 8, sources[1:])):
                for (ci, cj), aj in srcs:
                    rng = np.random.default_rng(71)  # the same global operands on every rank
                    a, b, c0 = operands(integers, rng, t, "N", n, k)
                    tri = in_triangle(uplo, n)
                    want = reference(t, two, "N", alpha, a, b, beta, c0).astype(dt)
                    c_in = np.where(tri, c0, np.nan).astype(dt)
                    la = np.asfortranarray(oracle.scatter(a, nb, nprow, npcol, ci, aj, extra_ld=1)[me])
                    lb = np.asfortranarray(oracle.scatter(b, nb, nprow, npcol, ci, aj, extra_ld=2)[me])
                    lc = np.asfortranarray(oracle.scatter(c_in, nb, nprow, npcol, ci, cj, extra_ld=3)[me])
                    lw = np.asfortranarray(oracle.scatter(want, nb, nprow, npcol, ci, cj)[me])
                    lt = np.asfortranarray(oracle.scatter(tri.astype(np.float64), nb, nprow, npcol, ci, cj)[me]) != 0
                    tag = f"{t} {'her2k' if two else 'herk'} uplo {uplo} k {k} C@({ci},{cj}) A@({ci},{aj}) grid {nprow}x{npcol}"
                    la_in, lb_in, lc_in = la.copy(order="F"), lb.copy(order="F"), lc.copy(order="F")

                    def check(got, what):
                        good = said(np.array_equal(got[lt], lw[lt]), f"{what}: local triangle differs ({tag})")
                        good &= said(got[~lt].tobytes() == lc_in[~lt].tobytes(), f"{what}: other triangle changed ({tag})")
                        return good

                    if two:
                        dlaf.hermitian_rank_2k_update(grid, uplo, "N", alpha, la, lb, beta, lc, nb, n=n, k=k, a_src=(ci, aj),
                                                      c_src=(ci, cj))
                    else:
                        dlaf.hermitian_rank_k_update(grid, uplo, "N", alpha, la, beta, lc, nb, n=n, k=k, a_src=(ci, aj),
                                                     c_src=(ci, cj))
                    ok &= check(lc, "host entry")
                    ok &= said(np.array_equal(la, la_in) and np.array_equal(lb, lb_in), f"host entry: A or B changed ({tag})")
                    # the resident entry
                    A = dlaf.GeneralDeviceMatrix(grid, dt, n, k, nb, ci, aj)
                    B = dlaf.GeneralDeviceMatrix(grid, dt, n, k, nb, ci, aj)
                    Cm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb, ci, cj)
                    A.upload(la)
                    B.upload(lb)
                    Cm.upload(lc_in)
                    if two:
                        dlaf.hermitian_rank_2k_update_device(uplo, "N", alpha, A, B, beta, Cm)
                    else:
                        dlaf.hermitian_rank_k_update_device(uplo, "N", alpha, A, beta, Cm)
                    got = lc_in.copy(order="F")
                    fa, fb = (np.zeros(x.shape, dtype=dt, order="F") for x in (la, lb))
                    Cm.download(got)
                    A.download(fa)
                    B.download(fb)
                    ok &= check(got, "resident entry")
                    ok &= said(np.array_equal(fa, la) and np.array_equal(fb, lb), f"resident entry: A or B changed ({tag})")
                    for h in (Cm, B, A):
                        h.close()
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("HERK_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
