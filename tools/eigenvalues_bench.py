"""Stage times of the routes to eigenvalues of a Hermitian matrix: the index range (0, 0) of hermitian_eigensolver (all n
eigenvalues out of the divide & conquer solver, no eigenvector: the only route before hermitian_eigenvalues existed),
the full solve, hermitian_eigenvalues (bisection on Sturm counts) for all n and for the lowest fractions, and the
by-value selection of the lowest 10 % beside the index-range call it resolves to.  One process, one GPU, host arrays;
per row one warm-up call, then `--reps` calls, each with its five stage times (eigensolver_profile(): HIP events around
each stage; stage 2 of a hermitian_eigenvalues row is the preparation and bisection kernels) and its wall time, and
their median.  The table goes to --out (default profiles/eigenvalues_bench.txt) and to stdout.

  python tools/eigenvalues_bench.py 20480 512 d
  python tools/eigenvalues_bench.py --root ../parent_checkout 20480 512 d      # the first two rows of another build"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

STAGES = ["reduction_to_band", "band_to_tridiagonal", "tridiagonal stage", "bt_band_to_tridiagonal", "bt_reduction_to_band"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("n", type=int)
    p.add_argument("nb", type=int)
    p.add_argument("dtype", choices=sorted(DT))
    p.add_argument("--fractions", type=float, nargs="*", default=[0.1, 0.01], help="each f runs the lowest f n eigenvalues")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--root", default=here)
    p.add_argument("--out", default=os.path.join(here, "profiles", "eigenvalues_bench.txt"))
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
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"eigenvalues_bench: {args.dtype} N={n} nb={nb} band={dlaf.get_band_size(nb)}, {dlaf.version()}")
    say(f"{'row':<34}" + "".join(f"{s:>24}" for s in STAGES) + f"{'stages total':>14}{'wall':>10}   (ms)")

    def row(name, call):
        runs, out = [], None
        for r in range(args.reps + 1):
            a = a0.copy(order="F")
            t0 = time.perf_counter()
            out = call(a)
            wall = (time.perf_counter() - t0) * 1e3
            ms = dlaf.eigensolver_profile()
            del a
            if r == 0:
                continue  # warm-up
            runs.append(ms + [sum(ms), wall])
            say(f"{name + ' #' + str(r):<34}" + "".join(f"{v:24.2f}" for v in ms) + f"{sum(ms):14.1f}{wall:10.1f}")
        med = [statistics.median(c) for c in zip(*runs)]
        tot = [x[5] for x in runs]
        say(f"{name + ' median':<34}" + "".join(f"{v:24.2f}" for v in med[:5]) + f"{med[5]:14.1f}{med[6]:10.1f}"
            f"   spread of the totals {max(tot) - min(tot):.1f}")
        return out, med

    (w_dc, _), m00 = row("eigensolver index (0, 0)", lambda a: dlaf.hermitian_eigensolver(grid, "L", a, nb, eigenvalues_index=(0, 0), z=z))
    row("eigensolver full", lambda a: dlaf.hermitian_eigensolver(grid, "L", a, nb, eigenvalues_index=(0, n), z=z))
    if not hasattr(dlaf, "hermitian_eigenvalues"):
        say("(this build has no hermitian_eigenvalues: the two rows above are all there is)")
    else:
        w_all, mall = row("eigenvalues all n", lambda a: dlaf.hermitian_eigenvalues(grid, "L", a, nb))
        say(f"  max |w_bisection - w_divide&conquer| / max|w| = {np.abs(w_all - w_dc).max() / np.abs(w_dc).max():.3e}")
        for f in args.fractions:
            k = max(1, min(n, int(round(f * n))))
            row(f"eigenvalues lowest {k} (f={f:g})", lambda a, k=k: dlaf.hermitian_eigenvalues(grid, "L", a, nb, eigenvalues_index=(0, k)))
        k = max(1, min(n - 1, int(round(0.1 * n))))
        vl, vu = float(w_dc[0]) - 1.0, float(w_dc[k - 1] + w_dc[k]) / 2
        (_, _, found), mval = row(f"eigensolver by value -> [0, {k})", lambda a: dlaf.hermitian_eigensolver(grid, "L", a, nb, eigenvalues_value=(vl, vu), z=z))
        _, midx = row(f"eigensolver index (0, {k})", lambda a: dlaf.hermitian_eigensolver(grid, "L", a, nb, eigenvalues_index=(0, k), z=z))
        say(f"  by value found {found}; wall by value - by index = {mval[6] - midx[6]:.1f} ms (the two-shift count launch "
            f"sits between stages 1 and 2, outside the stage times)")
        say(f"  tridiagonal stage, all n eigenvalues: bisection {mall[2]:.1f} ms, divide & conquer of the (0, 0) route "
            f"{m00[2]:.1f} ms; stages total {mall[5]:.1f} ms against {m00[5]:.1f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
