"""Worker of the distributed Hermitian multiplication test (tests/test_gpu_hermitian_multiplication.py): one process per
rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of dist_worker.py),
C = beta C + alpha A B / beta C + alpha B A on the grid gathered and compared with the analytic answer."""
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
    from test_gpu_hermitian_multiplication import DT, check_near, err_of, hermitian_system, scalars

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    ok = True
    sr, sc = max(0, nprow - 1), min(1, npcol - 1)   # the reference test's source process, for A, B and C
    # (t, m, n, mb, nb): the reference's shapes, MB != NB sets, a ragged multi-tile one
    sets = [("d", 19, 25, 6, 5), ("z", 15, 7, 3, 5), ("d", 70, 45, 8, 8), ("z", 37, 45, 8, 8), ("z", 7, 8, 2, 9)]
    for t, m, n, mb, nb in sets:
        dt = DT[t]
        alpha, beta = scalars(t)
        for side, uplo in itertools.product("LR", "LU"):
            a, b, c, res = hermitian_system(side, uplo, m, n, alpha, beta, dt)
            nba = mb if side == "L" else nb
            me = (grid.myrow, grid.mycol)
            la = np.asfortranarray(oracle.scatter(a, nba, nprow, npcol, sr, sc, extra_ld=1)[me])
            lb = np.asfortranarray(oracle.scatter_rect(b, mb, nb, nprow, npcol, sr, sc, extra_ld=2)[me])
            lc = np.asfortranarray(oracle.scatter_rect(c, mb, nb, nprow, npcol, sr, sc, extra_ld=3)[me])
            lb_in = lb.copy(order="F")
            dlaf.hermitian_multiplication(grid, side, uplo, alpha, la, lb, beta, lc, nba, m=m, n=n, a_src=(sr, sc),
                                          c_src=(sr, sc), c_block=(mb, nb))
            same_b = bool(np.array_equal(lb, lb_in))
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, (grid.myrow, grid.mycol, np.ascontiguousarray(lc), same_b))
            if rank == 0:
                got = oracle.gather_rect({(r, c_): np.asfortranarray(v) for r, c_, v, _ in parts}, m, n, mb, nb, nprow,
                                         npcol, sr, sc, dtype=dt)
                tol = 10 * (m + 1) * err_of(t)
                good, md = check_near(res, got, tol, tol)
                good = good and all(p[3] for p in parts)
                if not good:
                    print(f"[hemm_dist_worker] FAILED {t} {side}{uplo} {m}x{n} blocks {mb}x{nb} grid "
                          f"{nprow}x{npcol}: max diff {md} tol {tol}", flush=True)
                ok &= bool(good)
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("HEMM_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
