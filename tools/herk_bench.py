#!/usr/bin/env python3
"""Hermitian rank-k / rank-2k update timing on one GPU, one process, resident operands, device time (HIP events around
the sweep: dlaf_mi355x_multiplication_profile).  fp64 n = k = 16384, nb = 1024: herk N, herk C (T for real types) and
her2k N on a resident DeviceMatrix, with the yardstick beside them in the same rounds: general_multiplication_device with
B = A on a full general C for the same operand forms (N, T / N, C for herk N; T, N / C, N for herk C) -- existing code
that does the products of BOTH triangles.  Then complex double at 8192 (her2k with a complex alpha: the two-pass form).
The configurations of one type take turns inside every round, so a drift of the box reaches all of them alike; 3 warm-up
rounds, then 10 timed ones; median, minimum and maximum are reported, rates in TFlop/s of algorithmic flops: k n (n + 1)
for herk, twice that for her2k, 2 n n k for the GEMM (x4 complex).

    python tools/herk_bench.py [n_real] [n_complex] [nb]
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS = 3, 10
ALLOWANCE = 0.10  # herk may come out this far under the GEMM's rate for the same form (half the blocks: one partial
#                   round of resident workgroups in about 16, and diagonal blocks that compute a whole block for half)


def measure(dlaf, g, dt, n, nb):
    cx = np.dtype(dt).kind == "c"
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (n, n))
    if cx:
        x = x + 1j * rng.uniform(-1, 1, (n, n))
    x = np.asfortranarray(x.astype(dt))
    A, B, G = (dlaf.GeneralDeviceMatrix(g, dt, n, n, nb) for _ in range(3))
    H = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    for h in (A, B, G, H):
        h.upload(x)
    del x
    adj = "C" if cx else "T"
    alpha2 = dt(0.5 - 0.25j) if cx else dt(0.5)
    calls = {
        "herk N": lambda: dlaf.hermitian_rank_k_update_device("L", "N", 0.5, A, 0.25, H),
        "gemm N" + adj: lambda: dlaf.general_multiplication_device("N", adj, dt(0.5), A, A, dt(0.25), G),
        "herk " + adj: lambda: dlaf.hermitian_rank_k_update_device("L", adj, 0.5, A, 0.25, H),
        "gemm " + adj + "N": lambda: dlaf.general_multiplication_device(adj, "N", dt(0.5), A, A, dt(0.25), G),
        "her2k N": lambda: dlaf.hermitian_rank_2k_update_device("L", "N", alpha2, A, B, 0.25, H),
    }
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
        print(f"  {name:8s}: {med:9.3f} ms (min {lo:9.3f}, max {hi:9.3f})  {rates[name]:7.2f} TFlop/s "
              f"(best {flops[name] / lo / 1e9:7.2f})  flops {flops[name]:.4g}")
    for h in (A, B, G, H):
        h.close()
    return rates, adj


def main():
    args = [int(a) for a in sys.argv[1:]]
    n_real = args[0] if args else 16384
    n_cplx = args[1] if len(args) > 1 else 8192
    nb = args[2] if len(args) > 2 else 1024
    import dla_future_amd as dlaf
    dlaf.initialize()
    g = dlaf.Grid.single()
    print(f"hermitian_rank_k_update_device / hermitian_rank_2k_update_device beside general_multiplication_device (B = A, "
          f"full C), one process, resident operands; median of {REPS} rounds after {WARMUP} warm-up rounds, the "
          f"configurations taking turns in every round")
    for t, dt, n in (("d", np.float64, n_real), ("z", np.complex128, n_cplx)):
        print(f"{t} n = k = {n}, nb = {nb}")
        r, adj = measure(dlaf, g, dt, n, nb)
        for herk, gemm in (("herk N", "gemm N" + adj), ("herk " + adj, "gemm " + adj + "N"), ("her2k N", "gemm N" + adj)):
            ratio = r[herk] / r[gemm]
            verdict = "within" if ratio >= 1 - ALLOWANCE else "NOT within"
            print(f"{t}: {herk} / {gemm} = {ratio:.3f}: {verdict} {100 * ALLOWANCE:.0f} % below the GEMM's rate in this run")


if __name__ == "__main__":
    main()
