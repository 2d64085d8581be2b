"""Worker of the distributed general_addition / hermitian_complete test (tests/test_gpu_general_addition_grid.py): one
process per rank, every rank drives the same GPU through the host-staged transport over gloo (the pattern of
herk_dist_worker.py).  Exact operands -- integer entries in [-3, 3] -- at nb = 48 with m = 357, n = 165 (8 x 4 tiles:
more tile rows than process rows, classes of unequal length in the transposed panel, ragged last tiles) and non-zero
source processes, for d and z: op N, T, C with uplo A and L, hermitian_complete for both uplo and both kinds, both
conversions from a DeviceMatrix created with U; host and resident entries.  Every rank compares its own local part with
equality and everything else bit for bit.  The communication log shows that op N broadcasts nothing and that for op T
every member of a row / column communicator records the same sequence of broadcasts."""
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
    from test_gpu_general_addition import DT, in_part, integers, op_of, scalars
    from test_gpu_hermitian_complete import completed, triangle

    grid, _ = make_grid(dlaf, nprow, npcol, order)
    rank = dist.get_rank()
    me = (grid.myrow, grid.mycol)

    def said(cond, what):
        if not cond:
            print(f"[addition_dist_worker] rank {rank} {me}: FAILED {what}", flush=True)
        return bool(cond)

    def local(x, src, extra_ld=0):
        part = oracle.scatter(x, nb, nprow, npcol, src[0], src[1], extra_ld=extra_ld)[me]
        out = np.empty(part.shape, dtype=part.dtype, order="F")
        out[...] = part
        return out

    def same_sequences(events, what):
        """every member of my row communicator saw the same row broadcasts, of my column communicator the same column ones"""
        everyone = [None] * dist.get_world_size()
        dist.all_gather_object(everyone, (me, [e[:3] for e in events if e[0] in (0, 1)]))
        good = True
        for kind, axis in ((0, 0), (1, 1)):
            mine = [e for e in everyone[rank][1] if e[0] == kind]
            for (other, ev) in everyone:
                if other[axis] == me[axis]:
                    good &= said([e for e in ev if e[0] == kind] == mine, f"{what}: broadcast sequences of kind {kind} differ from {other}")
        return good, sum(len(ev) for _, ev in everyone)

    ok = True
    nb, m, n = 48, 357, 165
    r1, c1 = nprow - 1, npcol - 1
    c_src = (r1, c1)
    t_src = (0, c1 - 1 if npcol > 2 else 0)  # where A of op T / C starts: anywhere
    for t in ("d", "z"):
        dt = DT[t]
        alpha, beta = scalars(t)
        for op in ("N", "T", "C"):
            a_src = c_src if op == "N" else t_src
            for uplo in ("A", "L"):
                rng = np.random.default_rng(91)  # the same global operands on every rank
                a = integers(rng, t, (m, n) if op == "N" else (n, m))
                c0 = integers(rng, t, (m, n))
                part = in_part(uplo, m, n)
                want = (beta * c0 + alpha * op_of(op, a)).astype(dt)
                c_in = np.where(part, c0, np.nan).astype(dt)
                la, lc, lw = local(a, a_src, 1), local(c_in, c_src, 3), local(want, c_src)
                lp = local(part.astype(np.float64), c_src) != 0
                tag = f"{t} op {op} uplo {uplo} C@{c_src} A@{a_src} grid {nprow}x{npcol}"
                la_in, lc_in = la.copy(order="F"), lc.copy(order="F")

                def check(got, what):
                    good = said(np.array_equal(got[lp], lw[lp]), f"{what}: local part differs ({tag})")
                    good &= said(got[~lp].tobytes() == lc_in[~lp].tobytes(), f"{what}: outside the part changed ({tag})")
                    return good

                grid.comm_log(True)
                dlaf.general_addition(grid, uplo, op, alpha, la, beta, lc, nb, m=m, n=n, a_src=a_src, c_src=c_src)
                events = grid.comm_log_events()
                grid.comm_log(False)
                ok &= check(lc, "host entry")
                ok &= said(la.tobytes() == la_in.tobytes(), f"host entry: A changed ({tag})")
                if op == "N":
                    ok &= said(not [e for e in events if e[0] in (0, 1)], f"op N recorded a broadcast ({tag})")
                else:
                    good, total = same_sequences(events, tag)
                    ok &= good and said(total > 0, f"op {op} recorded no broadcast at all ({tag})")
                # the resident entry
                A = dlaf.GeneralDeviceMatrix(grid, dt, a.shape[0], a.shape[1], nb, *a_src)
                Cm = dlaf.GeneralDeviceMatrix(grid, dt, m, n, nb, *c_src)
                A.upload(la)
                Cm.upload(lc_in)
                dlaf.general_addition_device(uplo, op, alpha, A, beta, Cm)
                got, fa = lc_in.copy(order="F"), np.zeros(la.shape, dtype=dt, order="F")
                Cm.download(got)
                A.download(fa)
                ok &= check(got, "resident entry")
                ok &= said(fa.tobytes() == la.tobytes(), f"resident entry: A changed ({tag})")
                for h in (Cm, A):
                    h.close()
        # hermitian_complete and the conversions: square, order m
        for uplo in ("L", "U"):
            rng = np.random.default_rng(92)
            s0 = integers(rng, t, (m, m))
            tri = triangle(uplo, m)
            s_in = np.where(tri, s0, np.nan).astype(dt)
            ls_in = local(s_in, c_src, 2)
            ltri = local(tri.astype(np.float64), c_src) != 0
            for kind in ("H", "S"):
                tag = f"{t} complete uplo {uplo} kind {kind} @{c_src} grid {nprow}x{npcol}"
                lw = local(completed(t, uplo, kind, s_in), c_src)
                ls = ls_in.copy(order="F")
                dlaf.hermitian_complete(grid, uplo, kind, ls, nb, n=m, src=c_src)
                ok &= said(np.array_equal(ls, lw), f"host entry: wrong result ({tag})")
                G = dlaf.GeneralDeviceMatrix(grid, dt, m, m, nb, *c_src)
                G.upload(ls_in)
                dlaf.hermitian_complete_device(uplo, kind, G)
                got = np.zeros(ls_in.shape, dtype=dt, order="F")
                G.download(got)
                ok &= said(np.array_equal(got, lw), f"resident entry: wrong result ({tag})")
                keep = ltri if kind == "S" or t == "d" else local(triangle(uplo, m, True).astype(np.float64), c_src) != 0
                ok &= said(got[keep].tobytes() == ls_in[keep].tobytes(), f"resident entry: source triangle changed ({tag})")
                G.close()
        # both conversions from a DeviceMatrix created with U (it holds the transposed view on the device)
        rng = np.random.default_rng(93)
        s0 = integers(rng, t, (m, m))
        tri = triangle("U", m)
        s_in = np.where(tri, s0, np.nan).astype(dt)
        ltri = local(tri.astype(np.float64), c_src) != 0
        D = dlaf.DeviceMatrix(grid, dt, "U", m, nb, *c_src)
        G = dlaf.GeneralDeviceMatrix(grid, dt, m, m, nb, *c_src)
        D.upload(local(s_in, c_src))
        for kind in ("H", "T"):
            grid.comm_log(True)
            D.to_general(G, kind)
            events = grid.comm_log_events()
            grid.comm_log(False)
            got = np.zeros(ltri.shape, dtype=dt, order="F")
            G.download(got)
            ok &= said(np.array_equal(got, local(completed(t, "U", kind, s_in), c_src)), f"{t} to_general {kind} from U: wrong result")
            if kind == "T":
                ok &= said(not [e for e in events if e[0] in (0, 1)], "to_general T recorded a broadcast")
        b = integers(rng, t, (m, m))
        lb = local(b, c_src)
        G.upload(lb)
        D.from_general(G)
        got = np.full(ltri.shape, np.nan, dtype=dt, order="F")
        D.download(got)
        ok &= said(got[ltri].tobytes() == lb[ltri].tobytes() and np.isnan(got[~ltri]).all(), f"{t} from_general into U: wrong triangle")
        for h in (D, G):
            h.close()
    flags = [None] * dist.get_world_size()
    dist.all_gather_object(flags, ok)
    if rank == 0 and all(flags):
        print("ADDITION_WORKER_RESULT OK", flush=True)
    dist.destroy_process_group()
    sys.exit(0 if all(flags) else 1)


if __name__ == "__main__":
    main()
