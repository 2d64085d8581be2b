#!/usr/bin/env python3
"""Audit of the rotated fp64 slab (csrc/device/mma_core.hpp, mma_slab_rotated) in hipcc's -S output.

The slab reads its MFMA fragments with inline-assembly ds_read_b128 and waits for them with counted
s_waitcnt lgkmcnt(N).  hipcc regards the destination of such a read as written where the statement ends,
so nothing but register allocation keeps it from copying, spilling or reusing the registers while the read
is still in flight.  This script walks every function of an assembly file and reports

  * per basic block that holds MFMAs: the numbers of MFMAs, inline-asm LDS reads, direct-to-LDS loads,
    barriers, scalar loads and scratch accesses (the K loop must have no scratch access);
  * every instruction outside inline assembly that names a register of a read still in flight.  LDS reads
    return in order, so an asm "s_waitcnt lgkmcnt(N)" retires all but the N youngest; a compiler-made
    s_waitcnt with lgkmcnt(0) retires all.  An MFMA that READS an in-flight register is a violation; so is
    any other reader or writer.

usage: check_fragment_regs.py kernels_update.s [function-name-substring]
exit status 1 when a violation was found.
"""
import re
import sys


def regs_of(tok):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", tok):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "update_kernelId"
    func = None
    in_asm = False
    pending = []  # list of register sets, oldest first
    block = None
    stats = {}
    order = []
    bad = 0
    for ln, line in enumerate(open(path), 1):
        s = line.strip()
        m = re.match(r"^(\S+):\s*(;.*)?$", s)
        if m and not s.startswith(";"):
            name = m.group(1)
            if name.startswith("_Z") and want in name:
                func, pending, block = name, [], name
            elif name.startswith(".Lfunc_end"):
                if func and pending:
                    print(f"{func}: reads still in flight at the end of the function")
                    bad += 1
                func = None
            elif func:
                block = name
            continue
        if not func or not s:
            continue
        if s.startswith(";;#ASMSTART") or s.startswith(";#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND") or s.startswith(";#ASMEND"):
            in_asm = False
            continue
        if s.startswith(";") or s.startswith("."):
            continue
        op = s.split()[0]
        st = stats.setdefault((func, block), dict(mfma=0, asm_read=0, glds=0, barrier=0, s_load=0, scratch=0,
                                                  ds_other=0, first=ln))
        if (func, block) not in order:
            order.append((func, block))
        if op.startswith("v_mfma"):
            st["mfma"] += 1
        elif op.startswith("global_load_lds"):
            st["glds"] += 1
        elif op == "s_barrier":
            st["barrier"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            st["s_load"] += 1
        elif op.startswith("scratch_"):
            st["scratch"] += 1
        if in_asm:
            if op.startswith("ds_read"):
                st["asm_read"] += 1
                pending.append(regs_of(s.split(",")[0]))
            elif op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", s)
                if m:
                    n = int(m.group(1))
                    pending = pending[len(pending) - n:] if n else []
            continue
        if op.startswith("ds_"):
            st["ds_other"] += 1
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", s)
            if m and int(m.group(1)) == 0:
                pending = []
            continue
        if pending:
            flight = set().union(*pending)
            body = s.split(";")[0]
            ops = body[len(op):].split(",")
            if op.startswith("v_mfma"):
                # v_mfma D, A, B, C: D / C are accumulators, A / B the fragments
                used = regs_of(",".join(ops))
            else:
                used = regs_of(body)
            hit = used & flight
            if hit:
                print(f"{path}:{ln}: {func} [{block}]: `{body.strip()}` touches in-flight v{sorted(hit)}")
                bad += 1
    for key in order:
        st = stats[key]
        if st["mfma"]:
            f, b = key
            print(f"{f[:60]:60s} {b[:14]:14s} line {st['first']:7d}: mfma {st['mfma']:3d} asm_read {st['asm_read']:2d} "
                  f"glds {st['glds']:2d} barrier {st['barrier']} s_load {st['s_load']} ds_other {st['ds_other']} "
                  f"scratch {st['scratch']}")
    print("violations:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
