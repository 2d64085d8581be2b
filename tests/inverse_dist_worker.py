"""Worker of the distributed inverse test (tests/test_gpu_inverse_grid.py): one process per rank, every rank drives the
same GPU through the host-staged transport over gloo (the pattern of trmm_dist_worker.py).  triangular_inverse and
inverse_from_cholesky_factor on the grid; every rank checks ITS local part against the single-process wide-precision
reference of test_gpu_inverse.py with that file's bounds, and one singular operand must give every rank the same info."""
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
    import test_gpu_inverse as ti

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    me = (grid.myrow, grid.mycol)
    ok = True

    def local_of(full, nb, sr, sc):
        return np.asfortranarray(oracle.scatter(full, nb, nprow, npcol, sr, sc, extra_ld=2)[me])

    for t in "dz":
        for (n, nb) in [(400, 64), (333, 100)]:
            for (sr, sc) in [(0, 0), (min(1, nprow - 1), min(2, npcol - 1))]:
                for uplo in "LU":
                    tri, wref = ti.reference(t, n, uplo, "N")
                    _, a, mask = ti.padded(t, tri, uplo, "N")
                    full = np.asfortranarray(a)
                    inmask = local_of(mask.astype(np.float64), nb, sr, sc) > 0.5
                    for what in ("trtri", "potri"):
                        la = local_of(full, nb, sr, sc)
                        la0 = la.copy()
                        if what == "trtri":
                            info = dlaf.triangular_inverse(grid, uplo, "N", la, nb, isrc=sr, jsrc=sc, n=n)
                        else:
                            info = dlaf.inverse_from_cholesky_factor(grid, uplo, la, nb, isrc=sr, jsrc=sc, n=n)
                        good = info == 0 and np.array_equal(la[~inmask], la0[~inmask])
                        # the local part against the same part of a result that meets the bound exactly: put the
                        # local values into the reference's image and run the single-process check on it
                        if what == "trtri":
                            img = wref.astype(ti.DT[t])
                        else:
                            x = wref.conj().T @ wref if uplo == "L" else wref @ wref.conj().T
                            img = x.astype(ti.DT[t])
                        img = np.asfortranarray(np.where(mask, img, ti.SENTINEL).astype(ti.DT[t]))
                        limg = local_of(img, nb, sr, sc)
                        limg[inmask] = la[inmask]
                        locs = oracle.scatter(img, nb, nprow, npcol, sr, sc)
                        locs[me] = limg
                        mine = oracle.gather(locs, n, nb, nprow, npcol, sr, sc, dtype=ti.DT[t])
                        if what == "trtri":
                            r1 = ti.trtri_ratio(t, mine, tri, wref, mask)
                            good = good and r1 <= ti.C[t][0]
                            fig = (r1,)
                        else:
                            comp, p3 = ti.potri_ratios(t, mine, tri, wref, uplo)
                            good = good and comp <= ti.C[t][1] and p3 <= ti.C[t][2]
                            if t == "z":
                                good = good and bool((np.diagonal(mine).imag == 0).all())
                            fig = (comp, p3)
                        if not good:
                            print(f"[inverse_dist_worker] FAILED rank {me} {what} {t} {uplo} n={n} nb={nb} src=({sr},{sc}) "
                                  f"grid {nprow}x{npcol}: info {info} ratios {fig}", flush=True)
                        ok &= bool(good)
    # one singular operand: the same info on every rank, the local parts untouched
    t, n, nb, uplo, where = "d", 333, 100, "L", 205
    tri, _ = ti.reference(t, n, uplo, "N")
    _, a, _ = ti.padded(t, tri, uplo, "N")
    full = np.asfortranarray(a)
    full[where, where] = 0
    la = local_of(full, nb, 0, 0)
    la0 = la.copy()
    info = dlaf.triangular_inverse(grid, uplo, "N", la, nb, n=n)
    infos = [None] * dist.get_world_size()
    dist.all_gather_object(infos, int(info))
    if not (all(i == where + 1 for i in infos) and ti.same_bits(la, la0)):
        print(f"[inverse_dist_worker] FAILED singular case: infos {infos}", flush=True)
        ok = False
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if dist.get_rank() == 0 and all(flags):
        print("INVERSE_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
