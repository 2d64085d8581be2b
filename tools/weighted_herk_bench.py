#!/usr/bin/env python3
"""Timing of the weighted Hermitian rank-k update and of the matrix functions built on it, one GPU, one process, by the
method of tools/herk_bench.py: resident operands, device time from the profile hooks (HIP events around the sweep:
dlaf_mi355x_multiplication_profile; the eigensolver's five stages: dlaf_mi355x_eigensolver_profile), 3 warm-up and 10
timed rounds, the configurations taking turns inside every round, median (minimum, maximum).

Kernel benchmark: hermitian_weighted_rank_k_update_device beside hermitian_rank_k_update_device on the SAME operands,
fp64 n = k = 16384, nb = 1024, trans N and T; complex double at 8192, N and C.  The yardstick is herk in the same rounds;
the ratio weighted / herk of the rates is printed.  The weights cost BM * BK multiplies per slab against 2 * BM * BN * BK
MFMA flops; their upload (k reals) is enqueued before the timed window opens.

Function benchmark (--function): hermitian_power(-1/2) on a resident matrix, N = 20480, nb = 512, fp64 -- device time of
the eigensolver stages plus the weighted update -- beside (a) the eigensolver line plus a plain herk of that size, the
floor, and (b) the route offered before: the eigensolver with a host Z, a numpy column scaling, an upload, and
hermitian_rank_2k_update_device with the half-scaled copy (device times of eigensolver and her2k, and the wall time of
the whole route next to the wall time of hermitian_power_device).

    python tools/weighted_herk_bench.py [--function] [n_real] [n_complex] [nb]      (--function: [N] [nb] [warmup] [reps])
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS = 3, 10


def report(name, ms, flops=None):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    rate = f"  {flops / med / 1e9:7.2f} TFlop/s (best {flops / lo / 1e9:7.2f})" if flops else ""
    print(f"  {name:28s}: {med:10.3f} ms (min {lo:10.3f}, max {hi:10.3f}){rate}")
    return med


def kernel_benchmark(dlaf, g, dt, n, nb):
    cx = np.dtype(dt).kind == "c"
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (n, n))
    if cx:
        x = x + 1j * rng.uniform(-1, 1, (n, n))
    x = np.asfortranarray(x.astype(dt))
    d = rng.uniform(-1, 1, n).astype(np.float64)
    A = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
    H = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    A.upload(x)
    H.upload(x)
    del x
    adj = "C" if cx else "T"
    calls = {
        "herk N": lambda: dlaf.hermitian_rank_k_update_device("L", "N", 0.5, A, 0.25, H),
        "weighted N": lambda: dlaf.hermitian_weighted_rank_k_update_device("L", "N", 0.5, A, d, 0.25, H),
        "herk " + adj: lambda: dlaf.hermitian_rank_k_update_device("L", adj, 0.5, A, 0.25, H),
        "weighted " + adj: lambda: dlaf.hermitian_weighted_rank_k_update_device("L", adj, 0.5, A, d, 0.25, H),
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
    med = {name: report(name, ms[name], flops[name]) for name in calls}
    for op in ("N", adj):
        print(f"  weighted {op} / herk {op} = {med['herk ' + op] / med['weighted ' + op]:.3f} of herk's rate in the same rounds")
    for h in (A, H):
        h.close()


def function_benchmark(dlaf, g, n, nb, warmup, reps):
    dt = np.float64
    a = np.zeros((n, n), dtype=dt, order="F")
    dlaf.set_random_hermitian_positive_definite(g, a, n, nb)
    M = dlaf.DeviceMatrix(g, dt, "L", n, nb)
    Zg = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
    Zs = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
    keys = ("power: eigensolver", "power: weighted update", "power: device total", "power: wall", "floor: herk",
            "old: eigensolver", "old: her2k", "old: device total", "old: wall")
    ms = {k: [] for k in keys}
    z = np.zeros((n, n), dtype=dt, order="F")
    for r in range(warmup + reps):
        rec = {}
        # the new route, resident
        M.upload(a)
        t0 = time.perf_counter()
        w, dropped = dlaf.hermitian_power_device(M, -0.5)
        rec["power: wall"] = (time.perf_counter() - t0) * 1e3
        rec["power: eigensolver"] = float(sum(dlaf.eigensolver_profile()))
        rec["power: weighted update"] = dlaf.multiplication_profile()[0]
        rec["power: device total"] = rec["power: eigensolver"] + rec["power: weighted update"]
        # the route offered before: host Z, numpy scaling, upload, her2k with the half-scaled copy
        work = a.copy(order="F")
        t0 = time.perf_counter()
        w2 = dlaf.hermitian_eigensolver(g, "L", work, nb, z=z)[0]
        rec["old: eigensolver"] = float(sum(dlaf.eigensolver_profile()))
        half = np.asfortranarray(z * (0.5 * w2 ** -0.5)[None, :])
        Zg.upload(z)
        Zs.upload(half)
        dlaf.hermitian_rank_2k_update_device("L", "N", 1.0, Zg, Zs, 0.0, M)
        rec["old: her2k"] = dlaf.multiplication_profile()[0]
        rec["old: wall"] = (time.perf_counter() - t0) * 1e3
        rec["old: device total"] = rec["old: eigensolver"] + rec["old: her2k"]
        # the floor: a plain herk of that size on the resident Z
        dlaf.hermitian_rank_k_update_device("L", "N", 1.0, Zg, 0.0, M)
        rec["floor: herk"] = dlaf.multiplication_profile()[0]
        if r >= warmup:
            for k, v in rec.items():
                ms[k].append(v)
        del work, half
    med = {k: report(k, ms[k]) for k in keys}
    floor = med["power: eigensolver"] + med["floor: herk"]
    print(f"  hermitian_power device total / (its eigensolver + a plain herk) = {med['power: device total'] / floor:.3f}")
    print(f"  weighted update / plain herk = {med['power: weighted update'] / med['floor: herk']:.3f};  "
          f"weighted update / her2k of the old route = {med['power: weighted update'] / med['old: her2k']:.3f}")
    print(f"  wall: hermitian_power_device / old route = {med['power: wall'] / med['old: wall']:.3f}")
    for h in (M, Zg, Zs):
        h.close()


def main():
    fn = "--function" in sys.argv
    args = [int(a) for a in sys.argv[1:] if a != "--function"]
    import dla_future_amd as dlaf
    dlaf.initialize()
    g = dlaf.Grid.single()
    if fn:
        n = args[0] if args else 20480
        nb = args[1] if len(args) > 1 else 512
        warmup = args[2] if len(args) > 2 else WARMUP
        reps = args[3] if len(args) > 3 else REPS
        print(f"hermitian_power_device(-1/2), fp64 N = {n}, nb = {nb}, one process; median of {reps} rounds after {warmup} "
              f"warm-up rounds, the routes taking turns in every round; device times from the profile hooks, wall times beside")
        function_benchmark(dlaf, g, n, nb, warmup, reps)
        return
    n_real = args[0] if args else 16384
    n_cplx = args[1] if len(args) > 1 else 8192
    nb = args[2] if len(args) > 2 else 1024
    print(f"hermitian_weighted_rank_k_update_device beside hermitian_rank_k_update_device on the same operands, one process, "
          f"resident operands; median of {REPS} rounds after {WARMUP} warm-up rounds, the configurations taking turns in "
          f"every round")
    for t, dt, n in (("d", np.float64, n_real), ("z", np.complex128, n_cplx)):
        print(f"{t} n = k = {n}, nb = {nb}")
        kernel_benchmark(dlaf, g, dt, n, nb)


if __name__ == "__main__":
    main()
