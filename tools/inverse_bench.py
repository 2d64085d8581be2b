#!/usr/bin/env python3
"""Inverse timing on one GPU, resident operands, device time (HIP events: dlaf_mi355x_inverse_profile /
dlaf_mi355x_solver_profile).  Per configuration: triangular_inverse alone, the whole inverse_from_cholesky_factor, and
-- in the same process, on operands allocated before either route runs, the routes alternating -- the only route the
library offered before: potrs_device against a resident identity.  One warm-up, then the median of `reps` runs.

    python tools/inverse_bench.py [reps] [config ...]      config = d:16384:512 (type:N:nb); default: the three of
                                                           profiles/inverse_bench.txt
"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dla_future_amd as dlaf  # noqa: E402

PEAK_FP64_TFLOPS = 78.6
DT = {"d": np.float64, "z": np.complex128}


def run(g, t, n, nb, reps):
    dt = DT[t]
    a0 = np.zeros((n, n), dtype=dt, order="F")
    dlaf.set_random_hermitian_positive_definite(g, a0, n, nb)
    fac = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    work = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    rhs = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
    fac.upload(a0)
    del a0
    if fac.factorize() != 0:
        raise SystemExit("the factorization failed")
    eye = np.asfortranarray(np.eye(n, dtype=dt))
    cx = 4.0 if t == "z" else 1.0
    times = {"trtri": [], "potri": [], "potrs": []}
    for rep in range(reps + 1):
        work.copy_from(fac)
        assert work.invert_triangular("N") == 0
        ms_t, fl_t = dlaf.inverse_profile()
        work.copy_from(fac)
        assert work.invert_from_factor() == 0
        ms_p, fl_p = dlaf.inverse_profile()
        rhs.upload(eye)
        ms_s = 0.0
        for op in ("N", "C"):
            dlaf.triangular_solver_device("L", "L", op, "N", 1.0, fac, rhs)
            ms_s += dlaf.solver_profile()[0]
        if rep:  # the first round warms up
            times["trtri"].append(ms_t)
            times["potri"].append(ms_p)
            times["potrs"].append(ms_s)
    assert fl_t == cx * n ** 3 / 3 and fl_p == 2 * fl_t
    # spot check of the last results: a block of X A - I with X = the inverse, and the two routes against each other
    k = min(n, 256)
    x = np.zeros((n, n), dtype=dt, order="F")
    work.download(x)
    s = np.zeros((n, n), dtype=dt, order="F")
    rhs.download(s)
    diff = float(np.abs(np.tril(x)[:, :k] - np.tril(s)[:, :k]).max() / np.abs(s[:, :k]).max())
    md = {k_: statistics.median(v) for k_, v in times.items()}
    tf_t = fl_t / md["trtri"] / 1e9
    tf_p = fl_p / md["potri"] / 1e9
    print(f"{t} N={n} nb={nb} (median of {reps}):", flush=True)
    print(f"  triangular_inverse             {md['trtri']:9.2f} ms  {tf_t:6.2f} TFlop/s"
          + (f"  ({100 * tf_t / PEAK_FP64_TFLOPS:.1f} % of the fp64 peak)" if t == "d" else ""))
    print(f"  inverse_from_cholesky_factor   {md['potri']:9.2f} ms  {tf_p:6.2f} TFlop/s"
          + (f"  ({100 * tf_p / PEAK_FP64_TFLOPS:.1f} % of the fp64 peak)" if t == "d" else ""))
    print(f"  potrs_device against identity  {md['potrs']:9.2f} ms  -> the inverse is {md['potrs'] / md['potri']:.2f} x faster")
    print(f"  runs (ms): {times}")
    print(f"  the two routes differ by {diff:.2e} (relative, first {k} columns)", flush=True)
    for m in (fac, work, rhs):
        m.close()
    dlaf.release_workspace_pool()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cfgs = sys.argv[2:] or ["d:16384:512", "d:32768:1024", "z:8192:512"]
    dlaf.initialize()
    g = dlaf.Grid.single()
    for c in cfgs:
        t, n, nb = c.split(":")
        run(g, t, int(n), int(nb), reps)


if __name__ == "__main__":
    main()
