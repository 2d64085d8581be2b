"""Worker of the distributed weighted rank-k update / matrix function test (tests/test_gpu_weighted_rank_update_grid.py):
one process per rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of
herk_dist_worker.py).
  - the exact-operand weighted update, trans N, n = 357, k = 184, nb = 64 (three k tiles, the last one of 56: one step per
    tile, so the weight pointer advances per step), d and z, both uplo, zero and non-zero source processes, host and
    resident entries: every rank compares its local part of the triangle with equality, its part of the other triangle
    (NaN) bit for bit, and checks that its part of A did not change;
  - hermitian_function with x^(-1/2) at n = 150, nb = 32, d and z, against the reference and the bound of
    test_gpu_hermitian_function.py, every rank on its local part of the lower triangle; the other triangle (-9.9) bit for
    bit; all n eigenvalues on every rank."""
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
    from test_gpu_hermitian_rank_update import DT, in_triangle, integers, operands
    from test_gpu_weighted_rank_update import ALPHA, BETA, reference, weights
    import test_gpu_hermitian_function as hf

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    me = (grid.myrow, grid.mycol)

    def said(cond, what):
        """a check that would otherwise fail without a word: say which one (every rank, once)"""
        if not cond:
            print(f"[weighted_rank_update_dist_worker] rank {rank} {me}: FAILED {what}", flush=True)
        return bool(cond)

    ok = True
    nb, n, k = 64, 357, 184
    r1, c1 = nprow - 1, npcol - 1
    # (source of C, column source of A): A starts on C's process row; its columns elsewhere where there is room
    sources = [((0, 0), 0), ((r1, c1), c1 - 1 if npcol > 2 else c1)]
    for t in ("d", "z"):
        dt = DT[t]
        for uplo in ("L", "U"):
            for (ci, cj), aj in sources:
                rng = np.random.default_rng(91)  # the same global operands on every rank
                a, _, c0 = operands(integers, rng, t, "N", n, k)
                d = weights(rng, t, k)
                tri = in_triangle(uplo, n)
                want = reference(t, "N", ALPHA, a, d, BETA, c0).astype(dt)
                c_in = np.where(tri, c0, np.nan).astype(dt)
                la = np.asfortranarray(oracle.scatter(a, nb, nprow, npcol, ci, aj, extra_ld=1)[me])
                lc = np.asfortranarray(oracle.scatter(c_in, nb, nprow, npcol, ci, cj, extra_ld=3)[me])
                lw = np.asfortranarray(oracle.scatter(want, nb, nprow, npcol, ci, cj)[me])
                lt = np.asfortranarray(oracle.scatter(tri.astype(np.float64), nb, nprow, npcol, ci, cj)[me]) != 0
                tag = f"{t} weighted herk uplo {uplo} C@({ci},{cj}) A@({ci},{aj}) grid {nprow}x{npcol}"
                la_in, lc_in, d_in = la.copy(order="F"), lc.copy(order="F"), d.copy()

                def check(got, what):
                    good = said(np.array_equal(got[lt], lw[lt]), f"{what}: local triangle differs ({tag})")
                    good &= said(got[~lt].tobytes() == lc_in[~lt].tobytes(), f"{what}: other triangle changed ({tag})")
                    return good

                dlaf.hermitian_weighted_rank_k_update(grid, uplo, "N", ALPHA, la, d, BETA, lc, nb, n=n, k=k, a_src=(ci, aj),
                                                      c_src=(ci, cj))
                ok &= check(lc, "host entry")
                ok &= said(np.array_equal(la, la_in) and np.array_equal(d, d_in), f"host entry: A or d changed ({tag})")
                A = dlaf.GeneralDeviceMatrix(grid, dt, n, k, nb, ci, aj)
                Cm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb, ci, cj)
                A.upload(la)
                Cm.upload(lc_in)
                dlaf.hermitian_weighted_rank_k_update_device(uplo, "N", ALPHA, A, d, BETA, Cm)
                got = lc_in.copy(order="F")
                fa = np.zeros(la.shape, dtype=dt, order="F")
                Cm.download(got)
                A.download(fa)
                ok &= check(got, "resident entry")
                ok &= said(np.array_equal(fa, la), f"resident entry: A changed ({tag})")
                for h in (Cm, A):
                    h.close()

    # hermitian_function: S^(-1/2)
    n, nb = 150, 32
    f, fmax, lip = hf.FUNCS["rsqrt"]
    for t in ("d", "z"):
        dt = DT[t]
        for (ci, cj) in ((0, 0), (r1, c1)):
            a_in = hf.lower_input(t, n)
            want, wref = hf.reference(t, n, f)
            bnd = hf.bound(t, n, fmax, lip)
            la = np.asfortranarray(oracle.scatter(a_in, nb, nprow, npcol, ci, cj, extra_ld=2)[me])
            la_in = la.copy(order="F")
            lw = np.asfortranarray(oracle.scatter(want.astype(np.complex128 if t == "z" else np.float64), nb, nprow, npcol,
                                                  ci, cj)[me])
            lt = np.asfortranarray(oracle.scatter(in_triangle("L", n).astype(np.float64), nb, nprow, npcol, ci, cj)[me]) != 0
            tag = f"{t} hermitian_function rsqrt A@({ci},{cj}) grid {nprow}x{npcol}"
            w, sel = dlaf.hermitian_function(grid, "L", la, nb, f, isrc=ci, jsrc=cj, n=n)
            ok &= said(sel == (0, n), f"selection {sel} ({tag})")
            ok &= said(np.abs(w - wref).max() <= hf.bound(t, n, 0.0, 1.0), f"eigenvalues ({tag})")
            err = float(np.abs(la.astype(lw.dtype) - lw)[lt].max()) if lt.any() else 0.0
            ok &= said(err <= bnd, f"local triangle: err / bound {err / bnd:.3f} ({tag})")
            ok &= said(la[~lt].tobytes() == la_in[~lt].tobytes(), f"other triangle changed ({tag})")
            if t == "z":
                gi, gj = (np.asfortranarray(oracle.scatter(x.astype(np.float64), nb, nprow, npcol, ci, cj)[me])
                          for x in np.indices((n, n)))
                ok &= said((la.imag[(gi == gj)] == 0).all(), f"diagonal not exactly real ({tag})")
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("WEIGHTED_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
