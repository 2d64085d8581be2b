"""Worker of the distributed general multiplication test (tests/test_gpu_general_multiplication_grid.py): one process
per rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of dist_worker.py).
C = beta C + alpha A B (NoTrans x NoTrans, the SUMMA sweep) on exact operands -- integer entries in [-3, 3]; k = 170
(three k tiles at nb = 64) and k = 390 (2 kBuf + 1 = 7 k tiles with a ragged last one: the sweep's ring of kBuf = 3 operand
buffers is reused twice, so the wait that guards the reuse runs; the sums stay below 4 * 9 * 390, exact in fp64) --
through the host entry and the resident one; every rank compares its local part of C with equality and checks that its
parts of A and B did not change."""
import itertools
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
    from test_gpu_general_multiplication import DT, integers, reference, scalars

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    me = (grid.myrow, grid.mycol)

    def said(cond, what):
        """a check that would otherwise fail without a word: say which one (every rank, once)"""
        if not cond:
            print(f"[gemm_dist_worker] rank {rank} {me}: FAILED {what}", flush=True)
        return bool(cond)

    ok = True
    m, n, nb = 200, 150, 64
    r1, c1 = nprow - 1, npcol - 1
    # (source of C, column source of A, row source of B): A starts on C's process row, B on C's process column; the
    # last set has A's columns and B's rows start on different processes wherever the grid has room for it
    sources = [((0, 0), 0, 0), ((r1, c1), c1, r1), ((r1, 0), c1, 0)]
    for t in ("d", "z"):
        dt = DT[t]
        alpha, beta = scalars(t)
        for k, ((ci, cj), aj, bi) in itertools.product((170, 390), sources):
            rng = np.random.default_rng(41)  # the same global operands on every rank
            a, b, c0 = integers(rng, t, (m, k)), integers(rng, t, (k, n)), integers(rng, t, (m, n))
            want = reference(t, "N", "N", alpha, a, b, beta, c0).astype(dt)
            la = np.asfortranarray(oracle.scatter(a, nb, nprow, npcol, ci, aj, extra_ld=1)[me])
            lb = np.asfortranarray(oracle.scatter(b, nb, nprow, npcol, bi, cj, extra_ld=2)[me])
            lc = np.asfortranarray(oracle.scatter(c0, nb, nprow, npcol, ci, cj, extra_ld=3)[me])
            lw = np.asfortranarray(oracle.scatter(want, nb, nprow, npcol, ci, cj)[me])
            tag = f"{t} k {k} C@({ci},{cj}) A@({ci},{aj}) B@({bi},{cj}) grid {nprow}x{npcol}"
            la_in, lb_in, lc_in = la.copy(order="F"), lb.copy(order="F"), lc.copy(order="F")
            dlaf.general_multiplication(grid, "N", "N", alpha, la, lb, beta, lc, nb, m=m, n=n, k=k, a_src=(ci, aj),
                                        b_src=(bi, cj), c_src=(ci, cj))
            ok &= said(np.array_equal(lc, lw), f"host entry: local C differs ({tag})")
            ok &= said(np.array_equal(la, la_in) and np.array_equal(lb, lb_in), f"host entry: A or B changed ({tag})")
            # the resident entry
            A = dlaf.GeneralDeviceMatrix(grid, dt, m, k, nb, ci, aj)
            B = dlaf.GeneralDeviceMatrix(grid, dt, k, n, nb, bi, cj)
            Cm = dlaf.GeneralDeviceMatrix(grid, dt, m, n, nb, ci, cj)
            A.upload(la)
            B.upload(lb)
            Cm.upload(lc_in)
            dlaf.general_multiplication_device("N", "N", alpha, A, B, beta, Cm)
            got, fa, fb = (np.zeros(x.shape, dtype=dt, order="F") for x in (lc, la, lb))
            Cm.download(got)
            A.download(fa)
            B.download(fb)
            ok &= said(np.array_equal(got, lw), f"resident entry: local C differs ({tag})")
            ok &= said(np.array_equal(fa, la) and np.array_equal(fb, lb), f"resident entry: A or B changed ({tag})")
            for h in (Cm, B, A):
                h.close()
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("GEMM_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
