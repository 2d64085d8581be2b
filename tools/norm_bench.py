#!/usr/bin/env python3
"""Norm timing on one GPU, resident operands, device time (HIP events around each call: dlaf_mi355x_norm_profile).
fp64, N = 32768, nb = 512 by default: M, 1 and F of a general matrix and of a Hermitian one (lower triangle), 3 warm-ups
then 20 calls each, the median reported.  The yardstick runs in the same process over the allocation that holds the
general matrix: a read-only streaming kernel (tools/norm_stream.hip: 16-byte loads, one add per element, no structure);
its rate is the read rate this box reaches, and every norm is given as a ratio to it.  Last, what the route available
before costs: download of the matrix plus numpy.linalg.norm.

    python tools/norm_bench.py [N] [nb] [--build-only]
"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "tools", "norm_stream.hip")
LIB = os.path.join(ROOT, "tools", "norm_stream.so")
WARMUP, REPS = 3, 20


def build_yardstick():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-shared", "--offload-arch=gfx950",
                        SRC, "-o", LIB], check=True)
    return LIB


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    build_yardstick()
    if "--build-only" in sys.argv:
        return
    n = int(args[0]) if args else 32768
    nb = int(args[1]) if len(args) > 1 else 512
    import dla_future_amd as dlaf
    from dla_future_amd.capi import lib
    dlaf.initialize()
    g = dlaf.Grid.single()
    rng = np.random.default_rng(1)
    a = np.asfortranarray(rng.uniform(-1, 1, (n, n)))
    G = dlaf.GeneralDeviceMatrix(g, np.float64, n, n, nb)
    G.upload(a)
    H = dlaf.DeviceMatrix(g, np.float64, "L", n, nb)
    H.upload(a)

    def timed(call):
        ms = []
        for r in range(WARMUP + REPS):
            call()
            if r >= WARMUP:
                ms.append(dlaf.norm_profile())
        return statistics.median(m for m, _ in ms), min(m for m, _ in ms), ms[0][1]

    # the yardstick over the general matrix's own allocation
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert lib().dlaf_mi355x_gmatrix_device_tiles(G._h, C.byref(ptr), C.byref(nbytes)) == 0
    ys = C.CDLL(build_yardstick())
    ys.norm_stream_read.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    out = (C.c_float * REPS)()
    best = None
    for blocks in (2048, 4096, 8192, 16384):
        assert ys.norm_stream_read(ptr, nbytes.value, blocks, WARMUP, REPS, out) == 0
        med = statistics.median(out)
        print(f"yardstick, {blocks:5d} workgroups: {med:8.3f} ms  {nbytes.value / med / 1e6:8.1f} GB/s")
        best = med if best is None else min(best, med)
    yard = nbytes.value / best / 1e6
    print(f"yardstick (best launch width): {best:.3f} ms  {yard:.1f} GB/s over {nbytes.value} bytes")

    print(f"d N={n} nb={nb}: median of {REPS} calls after {WARMUP} warm-ups (min in brackets), GB/s of referenced bytes")
    for name, call_of in (("general", lambda nm: (lambda: dlaf.matrix_norm_device(nm, G))),
                          ("hermitian", lambda nm: (lambda: dlaf.matrix_norm_device(nm, H, "H")))):
        for nm in ("M", "1", "F"):
            med, mn, by = timed(call_of(nm))
            rate = by / med / 1e6
            print(f"  {name:9s} {nm}: {med:8.3f} ms ({mn:8.3f})  {rate:8.1f} GB/s  {rate / yard:5.2f} of the yardstick  "
                  f"({by:.0f} bytes)")
    # the route available before: download + numpy
    back = np.zeros((n, n), order="F")
    t0 = time.perf_counter()
    G.download(back)
    t1 = time.perf_counter()
    v = np.abs(back).max()
    t2 = time.perf_counter()
    f = np.linalg.norm(back)
    t3 = time.perf_counter()
    print(f"before this change: download {1e3 * (t1 - t0):.0f} ms + numpy max {1e3 * (t2 - t1):.0f} ms / numpy Frobenius "
          f"{1e3 * (t3 - t2):.0f} ms   (values {v:.6g} {f:.6g}; device {dlaf.matrix_norm_device('M', G):.6g} "
          f"{dlaf.matrix_norm_device('F', G):.6g})")


if __name__ == "__main__":
    main()
