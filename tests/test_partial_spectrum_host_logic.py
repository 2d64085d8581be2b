"""CPU tests of the host side of the partial-spectrum eigensolver entries (no GPU): every new entry is exported and typed,
the index arithmetic of the internal eigenvector matrix (dlaf_mi355x_partial_spectrum_plan: the global columns [b0, end)
with b0 = (begin / nb) nb, its column source rank, its local columns and where they sit in the caller's local array, the
pad columns [b0, begin)) agrees with a brute-force enumeration of owners and local indices over every process column,
and bad index ranges terminate before the GPU is touched."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KIND = {"s": "symmetric", "d": "symmetric", "c": "hermitian", "z": "hermitian"}
ENTRIES = [f"dlaf_{KIND[t]}_{name}_partial_spectrum_{t}" for t in "sdcz"
           for name in ("eigensolver", "generalized_eigensolver", "generalized_eigensolver_factorized")] + \
          [f"dlaf_p{t}{'syevd' if t in 'sd' else 'heevd'}_partial_spectrum" for t in "sdcz"] + \
          [f"dlaf_p{t}{'sygvd' if t in 'sd' else 'hegvd'}{f}_partial_spectrum" for t in "sdcz" for f in ("", "_factorized")] + \
          ["dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_s", "dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_d",
           "dlaf_mi355x_partial_spectrum_plan"]
GRIDS = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 2), (4, 6)]
SHAPES = [(1, 4), (6, 2), (19, 6), (34, 8), (70, 8), (333, 100)]


def ranges_of(n, nb):
    cand = [(0, 0), (0, 1), (0, n), (n - 1, n), (nb, 2 * nb), (nb + 1, n - 1), (1, 2)]
    return sorted({(b, e) for b, e in cand if 0 <= b <= e <= n})


def test_partial_spectrum_entries_exported():
    import inspect

    import dla_future_amd as d
    from dla_future_amd.capi import SIGNATURES
    L = C.CDLL(d.lib_path())
    for name in ENTRIES:
        assert hasattr(L, name) and name in SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "dlaf_mi355x", "dlaf_mi355x.h")).read()
    for name in ENTRIES:
        assert name + "(" in header, name
    for name in ("pxheevd_partial_spectrum", "partial_spectrum_plan"):
        assert callable(getattr(d, name)) and name in d.__all__, name
    for f in (d.hermitian_eigensolver, d.hermitian_generalized_eigensolver):
        assert {"eigenvalues_index", "z"} <= set(inspect.signature(f).parameters), f
    assert "eigenvalues_index" in inspect.signature(d.tridiagonal_eigensolver).parameters


@pytest.mark.parametrize("pr,pc", GRIDS)
def test_plan_against_enumeration(pr, pc):
    import dla_future_amd as d
    for (n, nb), z_jsrc in itertools.product(SHAPES, sorted({0, min(2, pc - 1)})):
        for begin, end in ranges_of(n, nb):
            seen = 0
            for c in range(pc):
                # the caller's local columns on process column c, in local order, as global columns
                mine = [j for j in range(n) if (j // nb + z_jsrc) % pc == c]
                wanted = [mine.index(j) for j in mine if begin <= j < end]
                b0, jsrc, ncl, first, pad = d.partial_spectrum_plan(n, nb, pc, c, z_jsrc, begin, end)
                assert b0 == (begin // nb) * nb and b0 <= begin < b0 + nb, (n, nb, begin, end)
                assert jsrc == (z_jsrc + begin // nb) % pc
                # the internal matrix: global columns [b0, end), tile g of it on process column (g + jsrc) % pc
                internal = [j for j in range(b0, end) if ((j - b0) // nb + jsrc) % pc == c]
                assert ncl == len(internal), (n, nb, pc, c, z_jsrc, begin, end)
                # it is the caller's distribution with whole tile columns dropped in front
                assert internal == [j for j in mine if b0 <= j < end]
                assert pad == sum(1 for j in internal if j < begin)
                assert pad == (begin - b0 if c == jsrc else 0) and pad <= ncl
                # the pad columns lead, and what follows them is exactly the wanted local columns, contiguous
                assert all(j < begin for j in internal[:pad]) and all(j >= begin for j in internal[pad:])
                assert list(range(first + pad, first + ncl)) == wanted, (n, nb, pc, c, z_jsrc, begin, end)
                if ncl:
                    assert mine[first:first + ncl] == internal
                seen += ncl - pad
            assert seen == end - begin


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "g = d.Grid.single(); n = 6\n"
           "a = np.eye(n, order='F'); b = np.eye(n, order='F'); z = np.zeros((n, n), order='F')\n")
NEEDLE = "must satisfy 0 <= begin <= end <= n"


# begin > end, end > n and a negative index through the main entry; one of them through each of the others
BAD_CALLS = [(c, b, e) for c, rs in [
    ("d.hermitian_eigensolver(g, 'L', a, 2, eigenvalues_index=(%d, %d), z=z)", [(3, 2), (0, 7), (-1, 2)]),
    ("d.hermitian_generalized_eigensolver(g, 'L', a, b, 2, eigenvalues_index=(%d, %d), z=z)", [(0, 7)]),
    ("d.hermitian_generalized_eigensolver(g, 'L', a, b, 2, factorized=True, eigenvalues_index=(%d, %d), z=z)", [(3, 2)]),
    ("d.tridiagonal_eigensolver(np.ones(n), np.ones(n - 1), 2, eigenvalues_index=(%d, %d), z=z)", [(-1, 2), (7, 7)]),
    ("d.partial_spectrum_plan(n, 2, 1, 0, 0, %d, %d)", [(3, 2)]),
] for b, e in rs]


@pytest.mark.parametrize("call,begin,end", BAD_CALLS)
def test_bad_ranges_terminate(call, begin, end):
    r = _run(PRELUDE + call % (begin, end) + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and NEEDLE in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("il,iu", [(0, 3), (3, 1), (1, 7)])  # 1-based inclusive: (1, 0) is the empty range
def test_bad_scalapack_ranges_terminate(il, iu):
    r = _run(PRELUDE + "desc = [1, g.context, n, n, 2, 2, 0, 0, n]\n"
             f"d.pxheevd_partial_spectrum('L', a, desc, z, desc, {il}, {iu}, n)\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and NEEDLE in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]
