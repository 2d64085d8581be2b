"""CPU tests of the C API's precondition layer (csrc/host/api_checks.hpp and the entries of c_api.cpp / c_api_host.cpp /
c_api_device.cpp that use it): every terminating check of the descriptor and ScaLAPACK entries that the other
host-logic files do not hold, and the return codes of the entries that answer a bad argument with a code.  Each
terminating case changes one argument of an otherwise valid 6 x 6 call with block 2 and expects the routine's message
on stderr before the GPU is touched (the checks run on a box without one).  A needle is the part of a message that
names the routine and the failed condition with its numbers; where a message exists in more than one wording across
the entries, the needle is a tuple of the fragments every wording has."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


SINGLE = "g = d.Grid.single()\n"
HOST_2X2 = "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)\n"

# one valid argument set for every entry below; a case mutates it after the grid exists
PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "L = lib()\n"
           "a = np.eye(6, order='F'); b = np.eye(6, order='F'); z = np.zeros((6, 6), order='F')\n"
           "rhs = np.ones((6, 4), order='F'); al = np.array([1.0])\n"
           "w = np.zeros(6); e = np.zeros(6); taus = np.zeros(6)\n"
           "pa, pb, pz, pw, pe, pt = (x.ctypes.data for x in (a, b, z, w, e, taus))\n"
           "da, db, dz, dc, dv = (DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6) for _ in range(5))\n"
           "dr = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n"
           "uplo = b'L'; band = 2; ldv = 6; ibtype = 1; ia = ja = ib = jb = iz = jz = 1\n"
           "info = C.c_int(0); m = C.c_int(0); begin = C.c_long(0); end = C.c_long(0)\n"
           "pinfo, pm, pbegin, pend = C.byref(info), C.byref(m), C.byref(begin), C.byref(end)\n"
           # trsm / trmm: B = rhs (6 x 4, dr); hemm: B = rhs (dr), C = c (drc)
           "side = b'L'; op = b'N'; diag = b'N'; be = np.array([0.5]); c = np.zeros((6, 4), order='F')\n"
           "drc = DLAFDescriptor(6, 4, 2, 2, 0, 0, 0, 0, 6)\n")
DESCS = ("ctx = g.context\n"
         "sa, sb, sz = ((C.c_int * 9)(1, ctx, 6, 6, 2, 2, 0, 0, 6) for _ in range(3))\n")

CALLS = {
    "cholesky": "L.dlaf_cholesky_factorization_d(ctx, uplo, pa, da)",
    "pdpotrf": "L.dlaf_pdpotrf(uplo, 6, pa, ia, ja, sa, pinfo)",
    "make_descriptor": "L.make_dlaf_descriptor(6, 6, ia, ja, sa)",
    "trsm": "L.dlaf_mi355x_triangular_solver_d(ctx, b'L', uplo, b'N', b'N', al.ctypes.data, pa, da, rhs.ctypes.data, dr)",
    "trsm_any": "L.dlaf_mi355x_triangular_solver_d(ctx, side, uplo, op, diag, al.ctypes.data, pa, da, rhs.ctypes.data, dr)",
    "trmm": "L.dlaf_mi355x_triangular_multiplication_d(ctx, side, uplo, op, diag, al.ctypes.data, pa, da, rhs.ctypes.data, "
            "dr)",
    "hemm": "L.dlaf_mi355x_hermitian_multiplication_d(ctx, side, uplo, al.ctypes.data, pa, da, rhs.ctypes.data, dr, "
            "be.ctypes.data, c.ctypes.data, drc)",
    "pdpotrs": "L.dlaf_mi355x_pdpotrs(uplo, 6, 6, pa, ia, ja, sa, pb, ib, jb, sb, pinfo)",
    "gen_to_std": "L.dlaf_mi355x_generalized_to_standard_d(ctx, uplo, pa, da, pb, db)",
    "pdhegst": "L.dlaf_mi355x_pdhegst(ibtype, uplo, 6, pa, ia, ja, sa, pb, ib, jb, sb, None, pinfo)",
    "red2band": "L.dlaf_mi355x_reduction_to_band_d(ctx, pa, da, band, pt)",
    "bt_red2band": "L.dlaf_mi355x_bt_reduction_to_band_d(ctx, band, pz, dc, pa, dv, pt)",
    "band_to_tridiag": "L.dlaf_mi355x_band_to_tridiagonal_d(ctx, pa, da, band, pw, pe, pz, ldv)",
    "eigensolver": "L.dlaf_symmetric_eigensolver_d(ctx, uplo, pa, da, pw, pz, dz)",
    "gen_eigensolver": "L.dlaf_symmetric_generalized_eigensolver_d(ctx, uplo, pa, da, pb, db, pw, pz, dz)",
    "eigenvalues": "L.dlaf_symmetric_eigenvalues_d(ctx, uplo, pa, da, pw, 0, 6)",
    "gen_eigenvalues": "L.dlaf_symmetric_generalized_eigenvalues_d(ctx, uplo, pa, da, pb, db, pw, 0, 6)",
    "by_value": "L.dlaf_symmetric_eigensolver_partial_spectrum_by_value_d(ctx, uplo, pa, da, pw, pz, dz, 0.0, 1.0, "
                "pbegin, pend)",
    "gen_by_value": "L.dlaf_symmetric_generalized_eigensolver_partial_spectrum_by_value_d(ctx, uplo, pa, da, pb, db, pw, "
                    "pz, dz, 0.0, 1.0, pbegin, pend)",
    "pdsyevd": "L.dlaf_pdsyevd(uplo, 6, pa, ia, ja, sa, pw, pz, iz, jz, sz, pinfo)",
    "pdsygvd": "L.dlaf_pdsygvd(uplo, 6, pa, ia, ja, sa, pb, ib, jb, sb, pw, pz, iz, jz, sz, pinfo)",
    "pdsyevd_eigenvalues": "L.dlaf_pdsyevd_eigenvalues(uplo, 6, pa, ia, ja, sa, pw, 1, 6, pinfo)",
    "pdsygvd_eigenvalues": "L.dlaf_pdsygvd_eigenvalues(uplo, 6, pa, ia, ja, sa, pb, ib, jb, sb, pw, 1, 6, pinfo)",
    "pdsyevd_by_value": "L.dlaf_pdsyevd_partial_spectrum_by_value(uplo, 6, pa, ia, ja, sa, pw, pz, iz, jz, sz, 0.0, 1.0, "
                        "pm, pinfo)",
    "pdsygvd_by_value": "L.dlaf_pdsygvd_partial_spectrum_by_value(uplo, 6, pa, ia, ja, sa, pb, ib, jb, sb, pw, pz, iz, jz, "
                        "sz, 0.0, 1.0, pm, pinfo)",
}


def _terminates(grid, entry, mutate, needle):
    r = _run(PRELUDE + grid + DESCS + f"{mutate}\n" + CALLS[entry] + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    for part in ((needle,) if isinstance(needle, str) else needle):
        assert part in r.stderr, (part, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


DTYPE = "(dtype) must be 1"
CONTEXTS = "live on different contexts"

TERMINATING = [
    # the reference's Cholesky entries
    ("cholesky", "uplo = b'Q'", "uplo must be 'L' or 'U', got 'Q'"),
    ("cholesky", "da.n = 5", "Cholesky needs a square matrix: 6 x 5"),
    ("cholesky", "da.mb = 3", "Cholesky needs square blocks: 3 x 2"),
    ("cholesky", "da.m = da.n = -1", "negative matrix size -1"),
    ("cholesky", "da.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    ("pdpotrf", "sa[0] = 2", DTYPE),
    ("pdpotrf", "ia = 2", ("ia", "ja", "must be 1")),
    ("make_descriptor", "ia = 2", "make_dlaf_descriptor: i = 2, j = 1 must be 1"),
    # p?potrs: the solver's prologue and its letter test (uplo U-or-not picks op 'C' for the first solve)
    ("pdpotrs", "ib = 2", "ia, ja, ib, jb must be 1"),
    ("pdpotrs", "sa[0] = 2", DTYPE),
    ("pdpotrs", "sb[1] = ctx - 1", ("A and B " + CONTEXTS, f"({2**31 - 1}, {2**31 - 2})")),
    ("pdpotrs", "uplo = b'Q'", "triangular solver: bad side/uplo/op/diag 'L' 'Q' 'C' 'N'"),
    # generalized to standard
    ("gen_to_std", "db.mb = db.nb = 3", "gen_to_std: A (6, block 2, source 0,0) and B (6, block 3, source 0,0) must be "
                                        "distributed alike"),
    ("gen_to_std", "uplo = b'Q'", "uplo must be 'L' or 'U', got 'Q'"),
    ("gen_to_std", "db.n = 5", "Cholesky needs a square matrix: 6 x 5"),
    ("gen_to_std", "da.isrc = db.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    ("pdhegst", "ibtype = 2", "p?hegst: only ibtype = 1 is built (got 2)"),
    ("pdhegst", "sb[0] = 2", DTYPE),
    ("pdhegst", "jb = 2", "ia, ja, ib, jb must be 1"),
    ("pdhegst", "sb[1] = ctx - 1", ("A and B " + CONTEXTS, f"({2**31 - 1}, {2**31 - 2})")),
    # reduction to band and its back-transformation, band to tridiagonal
    ("red2band", "band = 4", "reduction_to_band: band_size 4 must be >= 2 and divide the block size 2"),
    ("red2band", "band = 1", "reduction_to_band: band_size 1 must be >= 2 and divide the block size 2"),
    ("red2band", "da.jsrc = 1", "source rank (0,1) outside the 1 x 1 grid"),
    ("bt_red2band", "dv.isrc = 1", "bt_reduction_to_band: C (6 x 6, block 2 x 2, row source 0) must have V's block size 2, "
                                   "row count 6 and row source 1"),
    ("bt_red2band", "dc.mb = dc.nb = 3", "bt_reduction_to_band: C (6 x 6, block 3 x 3, row source 0) must have V's block "
                                         "size 2"),
    ("bt_red2band", "dc.jsrc = 1", "outside the 1 x 1 grid"),
    ("bt_red2band", "dv.jsrc = 1", "outside the 1 x 1 grid"),
    ("bt_red2band", "band = 4", "bt_reduction_to_band: band_size 4 must be >= 2 and divide the block size 2"),
    ("band_to_tridiag", "ldv = 3", "band_to_tridiagonal: ldv = 3 < n = 6"),
    ("band_to_tridiag", "band = 4", "band_to_tridiagonal: band_size 4 must be >= 2 and divide the block size 2"),
    ("band_to_tridiag", "da.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    # the eigensolver entries: Z (and B) described like A, sources inside the grid, the by-value outputs
    ("eigensolver", "dz.mb = dz.nb = 3", ("eigensolver: ", "must have A's size 6 x 6 and block 2 x 2")),
    ("eigensolver", "dz.i = 1", ("eigensolver: sub-matrix offsets", "must be 0")),
    ("eigensolver", "dz.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    ("gen_eigensolver", "dz.mb = dz.nb = 3", "gen_eigensolver: B and Z must have A's size 6 x 6 and block 2 x 2"),
    ("gen_eigensolver", "dz.j = 1", "gen_eigensolver: sub-matrix offsets must be 0"),
    ("gen_eigensolver", "db.n = 5", "Cholesky needs a square matrix: 6 x 5"),
    ("gen_eigensolver", "dz.jsrc = 1", "source rank (0,1) outside the 1 x 1 grid"),
    ("eigenvalues", "da.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    ("gen_eigenvalues", "db.mb = db.nb = 3", "gen_eigenvalues: B and Z must have A's size 6 x 6 and block 2 x 2"),
    ("gen_eigenvalues", "db.jsrc = 1", "source rank (0,1) outside the 1 x 1 grid"),
    ("by_value", "pend = None", "eigensolver: the by-value entries return their index range: begin, end must not be null"),
    ("by_value", "dz.mb = dz.nb = 3", "eigensolver: B and Z must have A's size 6 x 6 and block 2 x 2"),
    ("by_value", "dz.isrc = 2", "source rank (2,0) outside the 1 x 1 grid"),
    ("gen_by_value", "pbegin = None", "gen_eigensolver: the by-value entries return their index range: begin, end must "
                                      "not be null"),
    ("gen_by_value", "dz.mb = dz.nb = 3", "gen_eigensolver: B and Z must have A's size 6 x 6 and block 2 x 2"),
    # the ScaLAPACK argument lists of the eigensolver entries
    ("pdsyevd", "iz = 2", "ia, ja, iz, jz must be 1"),
    ("pdsyevd", "sz[0] = 2", DTYPE),
    ("pdsyevd", "sz[1] = ctx - 1", "A and Z " + CONTEXTS),
    ("pdsygvd", "jb = 2", "ia, ja, ib, jb, iz, jz must be 1"),
    ("pdsygvd", "sb[0] = 2", DTYPE),
    ("pdsygvd", "sz[1] = ctx - 1", CONTEXTS),
    ("pdsyevd_eigenvalues", "ja = 2", ("ia, ja", "must be 1")),
    ("pdsyevd_eigenvalues", "sa[0] = 2", DTYPE),
    ("pdsygvd_eigenvalues", "ib = 2", ("ia, ja, ib, jb", "must be 1")),
    ("pdsygvd_eigenvalues", "sb[1] = ctx - 1", CONTEXTS),
    ("pdsyevd_by_value", "iz = 2", ("ia, ja", "iz, jz must be 1")),
    ("pdsyevd_by_value", "sz[1] = ctx - 1", CONTEXTS),
    ("pdsygvd_by_value", "sz[0] = 2", DTYPE),
    ("pdsygvd_by_value", "jb = 2", "ia, ja, ib, jb, iz, jz must be 1"),
]


@pytest.mark.parametrize("entry,mutate,needle", TERMINATING)
def test_preconditions_terminate(entry, mutate, needle):
    _terminates(SINGLE, entry, mutate, needle)


@pytest.mark.parametrize("entry,mutate,needle", [
    ("trsm", "dr.isrc = 1", "triangular solver: A and B must share the source process along the triangular dimension"),
    ("gen_to_std", "da.isrc = 1", "gen_to_std: A (6, block 2, source 1,0) and B (6, block 2, source 0,0) must be "
                                  "distributed alike"),
    ("bt_red2band", "dv.isrc = 1", "bt_reduction_to_band: C (6 x 6, block 2 x 2, row source 0) must have V's block size 2, "
                                   "row count 6 and row source 1"),
    ("cholesky", "da.isrc = 1; da.jsrc = 2", "source rank (1,2) outside the 2 x 2 grid"),
    ("gen_eigensolver", "db.isrc = 1; dz.jsrc = -1", "source rank (0,-1) outside the 2 x 2 grid"),
])
def test_source_process_terminates(entry, mutate, needle):
    """On a 2 x 2 host grid (no broadcast is ever made) a source coordinate of 1 is inside the grid: the checks that
    compare the sources of two operands fire, and the grid's own bounds are the ones in the message."""
    _terminates(HOST_2X2, entry, mutate, needle)


# ---- triangular solver / multiplication and Hermitian multiplication: one case per terminating check of the descriptor
# entries, the full sentence each prints.  A is 6 x 6, B (and C) 6 x 4, block 2; side R cases shrink A to 4 x 4.
TRI = {"trsm_any": "triangular solver", "trmm": "triangular multiplication"}
TRI_CASES = [
    ("side = b'Q'", "{who}: bad side/uplo/op/diag 'Q' 'L' 'N' 'N'\n"),
    ("op = b'X'", "{who}: bad side/uplo/op/diag 'L' 'L' 'X' 'N'\n"),
    ("da.i = 1", "[dlaf_mi355x] sub-matrices are not supported: offsets must be 0\n"),
    ("dr.j = 1", "[dlaf_mi355x] sub-matrices are not supported: offsets must be 0\n"),
    ("da.n = 5", "{who}: A must be square with square blocks (6 x 5, 2 x 2)\n"),
    ("da.mb = 3", "{who}: A must be square with square blocks (6 x 6, 3 x 2)\n"),
    ("dr.m = 5", "{who}: A is 6 x 6, B is 5 x 4 (side L)\n"),
    ("side = b'R'", "{who}: A is 6 x 6, B is 6 x 4 (side R)\n"),
    ("dr.mb = 3", "{who}: B's blocks (3 x 2) do not match A's (2 x 2) for side L\n"),
    ("side = b'R'; da.m = da.n = 4; dr.nb = 3", "{who}: B's blocks (2 x 3) do not match A's (2 x 2) for side R\n"),
    ("da.isrc = 2", "[dlaf_mi355x] source rank (2,0) outside the 1 x 1 grid\n"),
    ("dr.jsrc = -1", "[dlaf_mi355x] source rank (0,-1) outside the 1 x 1 grid\n"),
]
TRI_SOURCE_CASES = [
    ("dr.isrc = 1", "{who}: A and B must share the source process along the triangular dimension\n"),
    ("side = b'R'; da.m = da.n = 4; da.jsrc = 1",
     "{who}: A and B must share the source process along the triangular dimension\n"),
]
HEMM = "[dlaf_mi355x] hermitian multiplication: "
HEMM_CASES = [
    ("side = b'Q'", HEMM + "bad side/uplo 'Q' 'L'\n"),
    ("uplo = b'Q'", HEMM + "bad side/uplo 'L' 'Q'\n"),
    ("da.j = 1", HEMM + "sub-matrices are not supported: offsets must be 0\n"),
    ("drc.i = 1", HEMM + "sub-matrices are not supported: offsets must be 0\n"),
    ("da.n = 5", HEMM + "A must be square with square blocks (6 x 5, 2 x 2)\n"),
    ("dr.n = 5", HEMM + "B (6 x 5, blocks 2 x 2) and C (6 x 4, blocks 2 x 2) differ\n"),
    ("drc.mb = 3", HEMM + "B (6 x 4, blocks 2 x 2) and C (6 x 4, blocks 3 x 2) differ\n"),
    ("dr.m = drc.m = 5", HEMM + "A is 6 x 6, B and C are 5 x 4 (side L)\n"),
    ("side = b'R'", HEMM + "A is 6 x 6, B and C are 6 x 4 (side R)\n"),
    ("dr.mb = drc.mb = 3", HEMM + "the blocks of B and C (3 x 2) do not match A's (2 x 2) for side L\n"),
    ("side = b'R'; da.m = da.n = 4; dr.nb = drc.nb = 3",
     HEMM + "the blocks of B and C (2 x 3) do not match A's (2 x 2) for side R\n"),
    ("da.isrc = 2", HEMM + "source rank (2,0) outside the 1 x 1 grid\n"),
]
HEMM_SOURCE_CASES = [
    ("dr.jsrc = 1", HEMM + "B and C must share the source process ((0,1) vs (0,0))\n"),
    ("drc.isrc = 1", HEMM + "B and C must share the source process ((0,0) vs (1,0))\n"),
    ("da.isrc = 1", HEMM + "A must share the source process of B and C along A's dimension\n"),
    ("side = b'R'; da.m = da.n = 4; da.jsrc = 1",
     HEMM + "A must share the source process of B and C along A's dimension\n"),
]


@pytest.mark.parametrize("mutate,needle", TRI_CASES)
@pytest.mark.parametrize("entry", sorted(TRI))
def test_triangular_preconditions_terminate(entry, mutate, needle):
    _terminates(SINGLE, entry, mutate, needle.format(who="[dlaf_mi355x] " + TRI[entry]))


@pytest.mark.parametrize("mutate,needle", TRI_SOURCE_CASES)
@pytest.mark.parametrize("entry", sorted(TRI))
def test_triangular_source_process_terminates(entry, mutate, needle):
    _terminates(HOST_2X2, entry, mutate, needle.format(who="[dlaf_mi355x] " + TRI[entry]))


@pytest.mark.parametrize("mutate,needle", HEMM_CASES)
def test_hermitian_multiplication_preconditions_terminate(mutate, needle):
    _terminates(SINGLE, "hemm", mutate, needle)


@pytest.mark.parametrize("mutate,needle", HEMM_SOURCE_CASES)
def test_hermitian_multiplication_source_process_terminates(mutate, needle):
    _terminates(HOST_2X2, "hemm", mutate, needle)


def _codes(body, expected):
    r = _run(PRELUDE + SINGLE + DESCS + "out = C.c_void_p(); bad = 12345\n"
             "def D(**kw):\n"
             "    x = DLAFDescriptor(6, 6, 2, 2, 0, 0, 0, 0, 6)\n"
             "    for k, v in kw.items(): setattr(x, k, v)\n"
             "    return x\n" + body + "\nprint('codes', *codes)")
    assert r.returncode == 0, (r.stdout, r.stderr[-800:])
    assert r.stdout.split() == ["codes"] + [str(c) for c in expected], r.stdout
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


def test_matrix_create_codes():
    _codes("f = L.dlaf_mi355x_matrix_create\n"
           "codes = [f(bad, b'd', b'L', D(), C.byref(out)), f(ctx, b'd', b'L', D(), None), f(bad, b'd', b'L', D(n=5), None),\n"
           "         f(ctx, b'd', b'L', D(n=5), C.byref(out)), f(ctx, b'd', b'L', D(mb=3), C.byref(out)),\n"
           "         f(ctx, b'd', b'L', D(i=1), C.byref(out)), f(ctx, b'd', b'L', D(isrc=2), C.byref(out)),\n"
           "         f(ctx, b'd', b'L', D(jsrc=-1), C.byref(out)), f(ctx, b'd', b'Q', D(), C.byref(out)),\n"
           "         f(ctx, b'd', b'Q', D(isrc=2), C.byref(out))]\n"
           "assert out.value is None",
           [-1, -1, -1, -3, -3, -3, -3, -3, -4, -3])


def test_gmatrix_create_codes():
    _codes("f = L.dlaf_mi355x_gmatrix_create\n"
           "codes = [f(bad, b'd', D(), C.byref(out)), f(ctx, b'd', D(), None), f(ctx, b'd', D(mb=3), C.byref(out)),\n"
           "         f(ctx, b'd', D(j=1), C.byref(out)), f(ctx, b'd', D(m=-1), C.byref(out)),\n"
           "         f(ctx, b'd', D(isrc=1), C.byref(out)), f(ctx, b'd', D(jsrc=-1), C.byref(out))]\n"
           "assert out.value is None",
           [-1, -1, -3, -3, -3, -3, -3])


def test_set_random_hpd_codes():
    _codes("f = L.dlaf_mi355x_set_random_hpd\n"
           "codes = [f(bad, b'd', pa, D(), 1), f(ctx, b'd', pa, D(n=5), 1), f(ctx, b'd', pa, D(mb=3), 1),\n"
           "         f(ctx, b'x', pa, D(), 1), f(bad, b'x', pa, D(n=5), 1)]",
           [-1, -3, -3, -2, -1])


def test_grid_entries_unknown_context_codes():
    _codes("other = d.Grid.single()\n"
           "buf = (C.c_long * 4)()\n"
           "codes = [L.dlaf_mi355x_grid_info(bad, None, None, None, None), L.dlaf_mi355x_grid_barrier(bad),\n"
           "         L.dlaf_mi355x_grid_selftest(bad, 64), L.dlaf_mi355x_grid_comm_log(bad, 1),\n"
           "         L.dlaf_mi355x_grid_comm_log_read(bad, buf, 1), L.dlaf_mi355x_grid_on_free(bad, None, None),\n"
           "         L.dlaf_mi355x_grid_rekey(bad, 7), L.dlaf_mi355x_grid_host_bcast(bad, 0, 0, None, 0),\n"
           "         L.dlaf_mi355x_grid_host_bcast(ctx, 2, 0, None, 0), L.dlaf_mi355x_grid_rekey(ctx, other.context),\n"
           "         L.dlaf_mi355x_grid_rekey(ctx, ctx), L.dlaf_mi355x_grid_info(ctx, None, None, None, None)]",
           [-1, -1, -1, -1, -1, -1, -1, -1, -1, -2, 0, 0])
