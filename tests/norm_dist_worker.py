"""Worker of the distributed norm test (tests/test_gpu_norms_grid.py): one process per rank, every rank drives the same
GPU through the host-staged transport over gloo (the pattern of inverse_dist_worker.py).  Every rank computes every norm
of every structure from ITS local part and checks: the exact operands of test_gpu_norms.py give the one-process numpy
reference (M, 1, I bit for bit, F within 2 ulp); the max norm of a uniform operand has the bits of a one-process run on
this rank; every rank reports the same bits for everything; a NaN that only the last rank owns reaches every rank."""
import os
import struct
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
    import test_gpu_norms as tn

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    single = dlaf.Grid.single()
    me = (grid.myrow, grid.mycol)
    ok = True
    record = []  # (what, bits of the value): must be the same list on every rank

    def local_of(full, nb, sr, sc):
        return oracle.scatter(np.asarray(full), nb, nprow, npcol, sr, sc, extra_ld=2)[me]

    def on_grid(norm, full, nb, combo, sr, sc):
        m, n = full.shape
        v = dlaf.matrix_norm(grid, norm, local_of(full, nb, sr, sc), nb, structure=combo[0], uplo=combo[1], diag=combo[2],
                             m=m, n=n, isrc=sr, jsrc=sc)
        record.append((norm, combo, full.shape, struct.pack("d", v)))
        return v

    def failed(msg):
        nonlocal ok
        ok = False
        print(f"[norm_dist_worker] FAILED rank {me} grid {nprow}x{npcol}: {msg}", flush=True)

    far = (nprow - 1, npcol - 1)  # (1, 2) on 2 x 3, (2, 1) on 3 x 2
    shapes = [((400, 400, 128), far), ((100, 100, 64), (0, 0)), ((400, 130, 128), far)]
    for t in "dc":
        for (m, n, nb), (sr, sc) in shapes:
            for combo in tn.COMBOS:
                if combo[0] != "G" and m != n:
                    continue
                a = tn.exact_operand(t, m, n, combo[0] == "H")
                ref = tn.exact_reference(a, *combo)
                for norm in tn.NORMS:
                    v = on_grid(norm, a, nb, combo, sr, sc)
                    try:
                        tn.assert_exact(t, norm, v, ref[norm], (t, combo, (m, n, nb), "grid"))
                    except AssertionError as e:
                        failed(f"exact operand: {e}")
        # the max norm of a uniform operand: the bits of a one-process run
        (m, n, nb), (sr, sc) = shapes[0]
        u = tn.uniform_operand(t, m, n)
        for combo in tn.COMBOS:
            v = on_grid("M", u, nb, combo, sr, sc)
            one = dlaf.matrix_norm(single, "M", u, nb, structure=combo[0], uplo=combo[1], diag=combo[2])
            if struct.pack("d", v) != struct.pack("d", one):
                failed(f"max norm {t} {combo}: grid {v!r} one process {one!r}")
        # a NaN in a tile that only the last rank owns (on or below the diagonal, so that every structure reads it)
        nt = -(-n // nb)
        gi, gj = next((i, j) for i in range(nt) for j in range(i + 1)
                      if (i + sr) % nprow == nprow - 1 and (j + sc) % npcol == npcol - 1)
        for combo in (tn.COMBOS[0], tn.COMBOS[1], tn.COMBOS[3]):
            b = np.array(tn.exact_operand(t, m, n, combo[0] == "H"), order="F")
            b[gi * nb + (3 if gi > gj else 5), gj * nb + 2] = np.nan
            for norm in tn.NORMS:
                v = on_grid(norm, b, nb, combo, sr, sc)
                if v == v:
                    failed(f"NaN of the last rank lost: {t} {combo} {norm} -> {v!r}")
    records = [None] * dist.get_world_size()
    dist.all_gather_object(records, record)
    if any(r != records[0] for r in records):
        bad = [(x, [struct.unpack("d", r[i][3])[0] for r in records]) for i, x in enumerate(records[0])
               if any(r[i] != x for r in records)]
        failed(f"ranks disagree: {bad[:5]}")
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if dist.get_rank() == 0 and all(flags):
        print("NORM_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
