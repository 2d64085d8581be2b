"""Worker of the distributed partial-spectrum test (tests/test_gpu_partial_spectrum_grid.py): one process per rank, every
rank drives the same GPU through the host-staged transport over gloo (the pattern of inverse_dist_worker.py).
hermitian_eigensolver and hermitian_generalized_eigensolver with an eigenvalue index range on the grid: w is the same on
every rank and bit-identical to the same grid's full call, the gathered columns [begin, end) meet the restated conditions
of test_gpu_partial_spectrum.py, and every rank's local store keeps its sentinels outside the wanted columns -- ranks that
own no wanted column and ranks that own only pad columns included.  DLAF_MI355X_DC_DIST_MIN=64 (set by the launcher
before the library loads) makes the tridiagonal solver split its root product over the ranks at these sizes."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PAD = -77.0  # what oracle.scatter fills the rows behind a local part with (extra_ld)


def main():
    nprow, npcol, order = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    assert os.environ.get("DLAF_MI355X_DC_DIST_MIN") == "64"
    dist.init_process_group("gloo")
    import dla_future_amd as dlaf
    from oracle import oracle
    from oracle import tridiag as td
    from dist_worker import make_grid
    import test_gpu_partial_spectrum as ps

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    me = (grid.myrow, grid.mycol)
    world = dist.get_world_size()
    ok = True

    def said(cond, what):
        if not cond:
            print(f"[partial_spectrum_dist_worker] rank {me}: FAILED {what}", flush=True)
        return bool(cond)

    def local_of(full, nb, sr, sc, extra_ld=0):
        return oracle.scatter(full, nb, nprow, npcol, sr, sc, extra_ld=extra_ld)[me]

    def everybody(obj):
        parts = [None] * world
        dist.all_gather_object(parts, obj)
        return parts

    def check_case(what, n, nb, dt, sr, zsc, begin, end, w, w_full, lz):
        """lz: this rank's local part of the sentinel-filled eigenvector matrix after the call (a view into its store)"""
        good = said(all(np.array_equal(w, x) for x in everybody(w)), f"{what}: w differs between ranks")
        good &= said(np.array_equal(w, w_full), f"{what}: w differs from the full call on the same grid")
        # my local elements: global column of each local column
        gcols = np.array([j for j in range(n) if (j // nb + zsc) % npcol == grid.mycol], dtype=int)
        wanted = (gcols >= begin) & (gcols < end)
        assert lz.shape[1] == len(gcols) or len(gcols) == 0
        if len(gcols):
            good &= said(bool(np.all(lz[:, ~wanted] == dt(ps.SENT))), f"{what}: a column outside [begin, end) was written")
        store = lz.base if lz.base is not None else lz
        good &= said(bool(np.all(store[lz.shape[0]:, :] == dt(PAD))), f"{what}: the rows behind the local part were written")
        parts = everybody((grid.myrow, grid.mycol, np.array(lz)))
        z = oracle.gather({(r, c): a for r, c, a in parts}, n, nb, nprow, npcol, sr, zsc, dtype=dt)
        return good, z

    # (type, n, nb, eigensolver_min_band, ranges): the issue's ranges, and one wide enough (>= 16 columns per rank) for
    # the root product of the restricted run to be split over the six ranks and all-gathered
    cases = [("d", 300, 64, 100, [(0, 40), (70, 110), (0, 300), (20, 230)]),
             ("z", 130, 32, 100, [(0, 40), (70, 110), (0, 130), (5, 125)]),
             ("s", 34, 8, 3, [(0, 40), (70, 110), (0, 34)])]
    for t, n, nb, b_min, ranges in cases:
        dt = ps.DT[t]
        a0 = ps.random_hermitian(n, dt, 700 + n)
        for sr, sc, zsc in [(0, 0, 0), (min(1, nprow - 1), min(1, npcol - 1), (min(1, npcol - 1) + 1) % npcol)]:
            dlaf.eigensolver_min_band(b_min)
            zshape = grid.local_shape(n, nb, sr, zsc)
            w_full, lz_full = dlaf.hermitian_eigensolver(grid, "L", np.asfortranarray(local_of(a0, nb, sr, sc)), nb, sr, sc, n=n,
                                                        z_jsrc=zsc, z_shape=zshape)
            for begin, end in ps.clamp(ranges, n):
                what = f"{t} n={n} nb={nb} src=({sr},{sc}) zsc={zsc} [{begin},{end}) grid {nprow}x{npcol}"
                lz = local_of(np.full((n, n), ps.SENT, dtype=dt, order="F"), nb, sr, zsc, extra_ld=2)
                w, _ = dlaf.hermitian_eigensolver(grid, "L", np.asfortranarray(local_of(a0, nb, sr, sc)), nb, sr, sc, n=n,
                                                  z_jsrc=zsc, eigenvalues_index=(begin, end), z=lz)
                good, z = check_case(what, n, nb, dt, sr, zsc, begin, end, w, w_full, lz)
                try:
                    ps.check_block(what, a0, w, z[:, begin:end], begin, dt)
                except AssertionError as e:
                    good = said(False, f"{what}: {e}")
                if (begin, end) == (0, n) and lz.size:
                    good &= said(np.array_equal(np.array(lz), lz_full), f"{what}: [0, n) differs from the old entry")
                ok &= bool(good)
            dlaf.eigensolver_min_band(100)

    # one generalized case
    t, n, nb, begin, end = "d", 130, 32, 5, 50
    dt = ps.DT[t]
    err = td.error_of(dt)
    a0 = ps.random_hermitian(n, dt, 900 + n)
    b0 = ps.random_hermitian(n, dt, 901 + n)
    b0 = np.asfortranarray((b0 @ b0.conj().T / n + 2 * np.eye(n)).astype(dt))
    what = f"generalized {t} n={n} nb={nb} [{begin},{end}) grid {nprow}x{npcol}"
    w_full, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", np.asfortranarray(local_of(a0, nb, 0, 0)),
                                                       np.asfortranarray(local_of(b0, nb, 0, 0)), nb, n=n)
    lz = local_of(np.full((n, n), ps.SENT, dtype=dt, order="F"), nb, 0, 0, extra_ld=2)
    w, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", np.asfortranarray(local_of(a0, nb, 0, 0)),
                                                  np.asfortranarray(local_of(b0, nb, 0, 0)), nb, n=n,
                                                  eigenvalues_index=(begin, end), z=lz)
    good, z = check_case(what, n, nb, dt, 0, 0, begin, end, w, w_full, lz)
    zk = z[:, begin:end]
    orth = float(np.abs(zk.conj().T @ b0 @ zk - np.eye(end - begin)).max())
    res = float(np.abs(a0 @ zk - (b0 @ zk) * w[None, begin:end]).max())
    good &= said(orth <= 10 * n * err * np.abs(b0).max(), f"{what}: B-orthonormality {orth}")
    good &= said(res <= 10 * n * err * max(1.0, np.abs(a0).max() * np.abs(w).max()), f"{what}: residual {res}")
    ok &= bool(good)

    flags = everybody(bool(ok))
    if dist.get_rank() == 0 and all(flags):
        print("PARTIAL_SPECTRUM_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
