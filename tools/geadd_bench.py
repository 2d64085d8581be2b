#!/usr/bin/env python3
"""general_addition / hermitian_complete / to_general timing on one GPU, resident operands, device time (HIP events
around each call: dlaf_mi355x_addition_profile), 3 warm-ups then 20 calls each, the median reported.  Cases: fp64
N = 32768 at nb = 512 and 1024, complex double N = 16384 at nb = 512; per case op N and op T with beta = 0 and beta != 0,
op C (complex), hermitian_complete in place and to_general('H').  The yardstick runs in the same process and rounds over
the same two allocations: a structure-free streaming copy with 16-byte loads and stores (tools/geadd_stream.hip), the
best of four launch widths; every case is given in GB/s of algorithmic bytes (read A + write C, + read C when
beta != 0; a completion reads and writes half the matrix) and as a ratio to it.  Last, once, what a transpose cost
before: download, numpy, upload.

    python tools/geadd_bench.py [--build-only] [--out FILE]
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
SRC = os.path.join(ROOT, "tools", "geadd_stream.hip")
LIB = os.path.join(ROOT, "tools", "geadd_stream.so")
WARMUP, REPS = 3, 20
CASES = [("d", np.float64, 32768, 512), ("d", np.float64, 32768, 1024), ("z", np.complex128, 16384, 512)]


def build_yardstick():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-shared", "--offload-arch=gfx950",
                        SRC, "-o", LIB], check=True)
    return LIB


def main():
    build_yardstick()
    if "--build-only" in sys.argv:
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import dla_future_amd as dlaf
    from dla_future_amd.capi import lib
    dlaf.initialize()
    g = dlaf.Grid.single()
    ys = C.CDLL(build_yardstick())
    ys.geadd_stream_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]

    def timed(call):
        ms = []
        for r in range(WARMUP + REPS):
            call()
            if r >= WARMUP:
                ms.append(dlaf.addition_profile())
        return statistics.median(m for m, _ in ms), min(m for m, _ in ms), ms[0][1]

    first = True
    for t, dt, n, nb in CASES:
        rng = np.random.default_rng(1)
        a = np.asfortranarray(rng.uniform(-1, 1, (n, n)).astype(dt))
        A = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
        Cm = dlaf.GeneralDeviceMatrix(g, dt, n, n, nb)
        A.upload(a)
        Cm.upload(a)
        pa, pc, nbytes = C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert lib().dlaf_mi355x_gmatrix_device_tiles(A._h, C.byref(pa), C.byref(nbytes)) == 0
        assert lib().dlaf_mi355x_gmatrix_device_tiles(Cm._h, C.byref(pc), C.byref(nbytes)) == 0
        out = (C.c_float * REPS)()
        best = None
        for blocks in (2048, 4096, 8192, 16384):
            assert ys.geadd_stream_copy(pc, pa, nbytes.value, blocks, WARMUP, REPS, out) == 0
            med = statistics.median(out)
            say(f"{t} N={n}: yardstick copy, {blocks:5d} workgroups: {med:8.3f} ms  {2 * nbytes.value / med / 1e6:8.1f} GB/s")
            best = med if best is None else min(best, med)
        yard = 2 * nbytes.value / best / 1e6
        say(f"{t} N={n} nb={nb}: yardstick (best launch width) {best:.3f} ms  {yard:.1f} GB/s (read + write of {nbytes.value} bytes); "
            f"median of {REPS} calls after {WARMUP} warm-ups (min in brackets)")
        D = dlaf.DeviceMatrix(g, dt, "L", n, nb)
        D.from_general(A)
        cases = [("op N beta 0", lambda: dlaf.general_addition_device("A", "N", 1.0, A, 0.0, Cm)),
                 ("op N beta 0 alpha 2", lambda: dlaf.general_addition_device("A", "N", 2.0, A, 0.0, Cm)),
                 ("op N beta 0.5", lambda: dlaf.general_addition_device("A", "N", 1.0, A, 0.5, Cm)),
                 ("op T beta 0", lambda: dlaf.general_addition_device("A", "T", 1.0, A, 0.0, Cm)),
                 ("op T beta 0.5", lambda: dlaf.general_addition_device("A", "T", 1.0, A, 0.5, Cm))]
        if t == "z":
            cases.append(("op C beta 0", lambda: dlaf.general_addition_device("A", "C", 1.0, A, 0.0, Cm)))
        cases += [("hermitian_complete L H", lambda: dlaf.hermitian_complete_device("L", "H", Cm)),
                  ("to_general H", lambda: D.to_general(Cm, "H"))]
        for name, call in cases:
            med, mn, by = timed(call)
            rate = by / med / 1e6
            say(f"  {name:24s}: {med:8.3f} ms ({mn:8.3f})  {rate:8.1f} GB/s  {rate / yard:5.2f} of the yardstick  ({by:.0f} bytes)")
        if first:
            # the route available before: download + numpy + upload
            first = False
            back = np.zeros((n, n), dtype=dt, order="F")
            t0 = time.perf_counter()
            A.download(back)
            t1 = time.perf_counter()
            tr = np.asfortranarray(back.T)
            t2 = time.perf_counter()
            Cm.upload(tr)
            t3 = time.perf_counter()
            say(f"  before this change, a transpose: download {1e3 * (t1 - t0):.0f} ms + numpy {1e3 * (t2 - t1):.0f} ms + upload "
                f"{1e3 * (t3 - t2):.0f} ms")
            del back, tr
        for h in (D, Cm, A):
            h.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
