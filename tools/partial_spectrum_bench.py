"""Stage times of hermitian_eigensolver for a partial spectrum: the old full entry first, then the partial-spectrum entry
with the eigenvalue index range [0, f n) for each fraction f.  One process, one GPU, host arrays (the wall time includes
the PCIe staging of A and of the wanted eigenvector columns); per row one warm-up call, then `--reps` calls, each printed
with its five stage times (eigensolver_profile(): HIP events around each stage) and its wall time, and their median.

  python tools/partial_spectrum_bench.py 20480 512 d 1.0 0.5 0.25 0.1
  python tools/partial_spectrum_bench.py --root ../parent_checkout 20480 512 d      # the full-entry row of another build

--root DIR imports dla_future_amd from DIR instead of this checkout: with no fractions only the old entry is called, so
the row can be taken on a commit that has no partial-spectrum entry."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

STAGES = ["reduction_to_band", "band_to_tridiagonal", "tridiagonal_eigensolver", "bt_band_to_tridiagonal",
          "bt_reduction_to_band"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("n", type=int)
    p.add_argument("nb", type=int)
    p.add_argument("dtype", choices=sorted(DT))
    p.add_argument("fractions", type=float, nargs="*", help="each f runs the range [0, f n)")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import dla_future_amd as dlaf

    n, nb, dt = args.n, args.nb, DT[args.dtype]
    dlaf.initialize()
    grid = dlaf.Grid.single()
    rng = np.random.default_rng(7)
    a0 = rng.uniform(-1, 1, (n, n)).astype(dt)
    if np.dtype(dt).kind == "c":
        a0 = a0 + 1j * rng.uniform(-1, 1, (n, n)).astype(dt)
    a0 = np.asfortranarray(np.tril(a0))  # only the lower triangle is referenced
    z = np.zeros((n, n), dtype=dt, order="F")
    print(f"partial_spectrum_bench: hermitian_eigensolver {args.dtype} N={n} nb={nb} band={dlaf.get_band_size(nb)}, "
          f"{dlaf.version()} from {os.path.dirname(dlaf.lib_path())}")
    print(f"{'row':<22}" + "".join(f"{s:>26}" for s in STAGES) + f"{'stages total':>14}{'wall':>10}   (ms)")

    def row(name, **kw):
        runs = []
        for r in range(args.reps + 1):
            a = a0.copy(order="F")
            t0 = time.perf_counter()
            w, _ = dlaf.hermitian_eigensolver(grid, "L", a, nb, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            ms = dlaf.eigensolver_profile()
            del a
            if r == 0:
                continue  # warm-up
            runs.append(ms + [sum(ms), wall])
            print(f"{name + ' #' + str(r):<22}" + "".join(f"{v:26.1f}" for v in ms) + f"{sum(ms):14.1f}{wall:10.1f}", flush=True)
        med = [statistics.median(c) for c in zip(*runs)]
        tot = [x[5] for x in runs]
        print(f"{name + ' median':<22}" + "".join(f"{v:26.1f}" for v in med[:5]) + f"{med[5]:14.1f}{med[6]:10.1f}"
              f"   spread of the totals {max(tot) - min(tot):.1f}", flush=True)
        return w

    w_full = row("full entry")
    for f in args.fractions:
        end = max(0, min(n, int(round(f * n))))
        w = row(f"[0, {end}) f={f:g}", eigenvalues_index=(0, end), z=z)
        if not np.array_equal(w, w_full):
            print(f"  eigenvalues differ from the full entry's: max {np.abs(w - w_full).max():.3e}")


if __name__ == "__main__":
    main()
