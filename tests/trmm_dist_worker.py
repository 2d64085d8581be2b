"""Worker of the distributed triangular multiplication test (tests/test_gpu_triangular_multiplication.py): one
process per rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of
dist_worker.py), B = alpha op(A) B on the grid gathered and compared with the analytic answer."""
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

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    ok = True
    sr, sc = max(0, nprow - 1), min(1, npcol - 1)   # the reference test's source process
    # (t, m, n, mb, nb): the reference's shapes (analytic), a ragged multi-tile one, MB != NB
    sets = [("d", 19, 25, 6, 6), ("z", 15, 7, 3, 3), ("d", 70, 45, 8, 8), ("z", 19, 25, 6, 5), ("d", 15, 7, 3, 5)]
    for t, m, n, mb, nb in sets:
        dt = oracle.DTYPES[t]
        alpha = dt(complex(-1.2, .7)) if t in "cz" else dt(-1.2)
        for side, uplo, op, diag in itertools.product("LR", "LU", "NTC", "NU"):
            # op(A) X = B / alpha  <=>  B = alpha op(A) X: the input is X, the expected result B
            a, b, x = oracle.triangular_system(side, uplo, op, diag, 1 / alpha, m, n, dt)
            nba = mb if side == "L" else nb
            bsr, bsc = (sr, 0) if side == "L" else (0, sc)
            la = np.asfortranarray(oracle.scatter(a, nba, nprow, npcol, sr, sc, extra_ld=1)[(grid.myrow, grid.mycol)])
            lb = np.asfortranarray(oracle.scatter_rect(x, mb, nb, nprow, npcol, bsr, bsc, extra_ld=2)[(grid.myrow, grid.mycol)])
            dlaf.triangular_multiplication(grid, side, uplo, op, diag, alpha, la, lb, nba, m=m, n=n, a_src=(sr, sc),
                                           b_src=(bsr, bsc), b_block=(mb, nb))
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, (grid.myrow, grid.mycol, np.ascontiguousarray(lb)))
            if rank == 0:
                got = oracle.gather_rect({(r, c): np.asfortranarray(v) for r, c, v in parts}, m, n, mb, nb, nprow, npcol,
                                         bsr, bsc, dtype=dt)
                tol = 40 * (m + 1) * (8 if t in "cz" else 2) * oracle.eps_of(dt)
                good, md = oracle.check_near(b, got, tol, tol)
                if not good:
                    print(f"[trmm_dist_worker] FAILED {t} {side}{uplo}{op}{diag} {m}x{n} blocks {mb}x{nb} grid "
                          f"{nprow}x{npcol}: max diff {md} tol {tol}", flush=True)
                ok &= bool(good)
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("TRMM_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
