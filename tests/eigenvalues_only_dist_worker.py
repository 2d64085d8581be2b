"""Worker of the distributed eigenvalues-only / by-value test (tests/test_gpu_eigenvalues_only_grid.py): one process per
rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of
partial_spectrum_dist_worker.py), at that worker's smallest multi-tile size (n = 34, nb = 8, eigensolver_min_band = 3).
hermitian_eigenvalues: w the same bits on every rank, within n error max|lambda| of the prescribed spectrum, a range
call writes its slice alone.  hermitian_eigensolver(eigenvalues_value=...): (begin, end) and w the same on every rank,
(begin, end) the count from the prescribed spectrum, the gathered columns [begin, end) through the residual and
orthogonality check of test_gpu_partial_spectrum.py, sentinels kept everywhere else."""
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
    dist.init_process_group("gloo")
    import dla_future_amd as dlaf
    from oracle import oracle
    from oracle import tridiag as td
    from dist_worker import make_grid
    import test_gpu_eigenvalues_only as eo
    import test_gpu_partial_spectrum as ps

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    me = (grid.myrow, grid.mycol)
    world = dist.get_world_size()
    ok = True

    def said(cond, what):
        if not cond:
            print(f"[eigenvalues_only_dist_worker] rank {me}: FAILED {what}", flush=True)
        return bool(cond)

    def local_of(full, nb, sr, sc, extra_ld=0):
        return oracle.scatter(full, nb, nprow, npcol, sr, sc, extra_ld=extra_ld)[me]

    def everybody(obj):
        parts = [None] * world
        dist.all_gather_object(parts, obj)
        return parts

    n, nb, b_min = 34, 8, 3
    for t in ("d", "z", "s"):
        dt = eo.DT[t]
        rt = np.zeros(0, dtype=dt).real.dtype
        a0, _, lam = eo.problem(n, t)
        bar = n * td.error_of(dt) * np.abs(lam).max()
        for sr, sc, zsc in [(0, 0, 0), (min(1, nprow - 1), min(1, npcol - 1), (min(1, npcol - 1) + 1) % npcol)]:
            dlaf.eigensolver_min_band(b_min)
            what = f"{t} n={n} nb={nb} src=({sr},{sc}) zsc={zsc} grid {nprow}x{npcol}"
            # ---- eigenvalues only
            w = dlaf.hermitian_eigenvalues(grid, "L", np.asfortranarray(local_of(a0, nb, sr, sc)), nb, sr, sc, n=n)
            good = said(all(np.array_equal(w, x) for x in everybody(w)), f"{what}: eigenvalues differ between ranks")
            good &= said(dlaf.eigensolver_profile()[3:5] == [0, 0], f"{what}: stages 3-4 not zero")
            diff = float(np.abs(w - lam).max())
            good &= said(diff <= bar and bool(np.all(np.diff(w) >= 0)), f"{what}: eigenvalues off the spectrum: {diff} > {bar}")
            out = np.full(n, eo.SENT, dtype=rt)
            dlaf.hermitian_eigenvalues(grid, "L", np.asfortranarray(local_of(a0, nb, sr, sc)), nb, sr, sc, n=n,
                                       eigenvalues_index=(5, 20), w=out)
            good &= said(np.array_equal(out[5:20], w[5:20]) and bool(np.all(out[:5] == rt.type(eo.SENT))) and
                         bool(np.all(out[20:] == rt.type(eo.SENT))), f"{what}: the range call")
            # ---- by value
            vl, vu, begin, end = eo.intervals(lam)[4]
            lz = local_of(np.full((n, n), eo.SENT, dtype=dt, order="F"), nb, sr, zsc, extra_ld=2)
            wv, _, found = dlaf.hermitian_eigensolver(grid, "L", np.asfortranarray(local_of(a0, nb, sr, sc)), nb, sr, sc,
                                                      n=n, z_jsrc=zsc, eigenvalues_value=(vl, vu), z=lz)
            good &= said(all(x == found for x in everybody(found)), f"{what}: (begin, end) differs between ranks")
            good &= said(found == (begin, end), f"{what}: (begin, end) = {found}, the spectrum says {(begin, end)}")
            good &= said(all(np.array_equal(wv, x) for x in everybody(wv)), f"{what}: w differs between ranks")
            diff = float(np.abs(wv - lam).max())
            good &= said(diff <= bar, f"{what}: w off the spectrum: {diff} > {bar}")
            gcols = np.array([j for j in range(n) if (j // nb + zsc) % npcol == grid.mycol], dtype=int)
            wanted = (gcols >= begin) & (gcols < end)
            if len(gcols):
                good &= said(bool(np.all(lz[:, ~wanted] == dt(eo.SENT))), f"{what}: a column outside [begin, end) was written")
            store = lz.base if lz.base is not None else lz
            good &= said(bool(np.all(store[lz.shape[0]:, :] == dt(PAD))), f"{what}: the rows behind the local part were written")
            parts = everybody((grid.myrow, grid.mycol, np.array(lz)))
            z = oracle.gather({(r, c): a for r, c, a in parts}, n, nb, nprow, npcol, sr, zsc, dtype=dt)
            try:
                ps.check_block(what, a0, wv, z[:, begin:end], begin, dt)
            except AssertionError as e:
                good = said(False, f"{what}: {e}")
            ok &= bool(good)
            dlaf.eigensolver_min_band(100)

    flags = everybody(bool(ok))
    if dist.get_rank() == 0 and all(flags):
        print("EIGENVALUES_ONLY_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
