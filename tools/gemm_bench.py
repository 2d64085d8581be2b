#!/usr/bin/env python3
"""General multiplication timing on one GPU, one process, resident operands, device time (HIP events around the sweep:
dlaf_mi355x_multiplication_profile).  fp64 m = n = k = 16384, nb = 1024 for NN, NT, TN and TT, with the yardstick beside
them in the same process: hermitian_multiplication_device (side R, uplo L -- its canonical form, no adjoint copies) at
m = n = 16384, the existing kernel that does the same work per tile plus the triangle fetch and a read-modify-write of C
per k tile.  Then complex double at 8192 (NN, NC, CN, CC and the same yardstick).  The configurations of one type take
turns inside every repetition, so a drift of the box reaches all of them alike; 3 warm-up rounds, then 10 timed ones;
median, minimum and maximum are reported, rates in TFlop/s of algorithmic flops (2 m n k, x4 complex).

    python tools/gemm_bench.py [n_real] [n_complex] [nb]
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS = 3, 10
TOLERANCE = 0.03  # NN may come out this far under the yardstick's rate


def measure(dlaf, g, dt, n, nb, forms):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (n, n))
    if np.dtype(dt).kind == "c":
        x = x + 1j * rng.uniform(-1, 1, (n, n))
    x = np.asfortranarray(x.astype(dt))
    A, B, Cm = (dlaf.GeneralDeviceMatrix(g, dt, n, n, nb) for _ in range(3))
    H = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    for h in (A, B, Cm, H):
        h.upload(x)
    del x
    alpha, beta = dt(0.5), dt(0.25)
    calls = {f: (lambda f=f: dlaf.general_multiplication_device(f[0], f[1], alpha, A, B, beta, Cm)) for f in forms}
    calls["hemm"] = lambda: dlaf.hermitian_multiplication_device("R", "L", alpha, H, B, beta, Cm)
    ms = {name: [] for name in calls}
    flops = {}
    for r in range(WARMUP + REPS):
        for name, call in calls.items():
            call()
            t, fl = dlaf.multiplication_profile()
            flops[name] = fl
            if r >= WARMUP:
                ms[name].append(t)
    rates = {}
    for name in calls:
        med, lo, hi = statistics.median(ms[name]), min(ms[name]), max(ms[name])
        rates[name] = flops[name] / med / 1e9
        print(f"  {name:5s}: {med:9.3f} ms (min {lo:9.3f}, max {hi:9.3f})  {rates[name]:7.2f} TFlop/s "
              f"(best {flops[name] / lo / 1e9:7.2f})  flops {flops[name]:.4g}")
    for h in (A, B, Cm, H):
        h.close()
    return rates


def main():
    args = [int(a) for a in sys.argv[1:]]
    n_real = args[0] if args else 16384
    n_cplx = args[1] if len(args) > 1 else 8192
    nb = args[2] if len(args) > 2 else 1024
    import dla_future_amd as dlaf
    dlaf.initialize()
    g = dlaf.Grid.single()
    print(f"general_multiplication_device beside hermitian_multiplication_device (R, L), one process, resident operands; "
          f"median of {REPS} rounds after {WARMUP} warm-up rounds, the configurations taking turns in every round")
    print(f"d m = n = k = {n_real}, nb = {nb}")
    rd = measure(dlaf, g, np.float64, n_real, nb, ["NN", "NT", "TN", "TT"])
    print(f"z m = n = k = {n_cplx}, nb = {nb}")
    rz = measure(dlaf, g, np.complex128, n_cplx, nb, ["NN", "NC", "CN", "CC"])
    for t, r in (("d", rd), ("z", rz)):
        ratio = r["NN"] / r["hemm"]
        verdict = "within" if ratio >= 1 - TOLERANCE else "NOT within"
        print(f"{t}: NN / hemm = {ratio:.3f}: NN is {verdict} {100 * TOLERANCE:.0f} % of the Hermitian multiplication's rate "
              f"in this run")
        for f, v in r.items():
            if f not in ("NN", "hemm"):
                print(f"{t}: {f} / hemm = {v / r['hemm']:.3f}")


if __name__ == "__main__":
    main()
