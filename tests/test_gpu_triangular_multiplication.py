"""Triangular multiplication on the GPU: B = alpha op(A) B / alpha B op(A) against the reference's analytic systems
(test/unit/multiplication/test_multiplication_triangular.cpp: getTriangularSystem with 1 / alpha, so that the input
is X and the expected result B, at the reference's tolerance), against float64 / complex128 products of random
operands on multi-tile shapes, on resident operands, through p?trmm, round-tripped through the solver, in the
miniapp and on grids."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["s", "d", "c", "z"]
VARIANTS = list(itertools.product("LR", "LU", "NTC", "NU"))
# test_multiplication_triangular.cpp: (m, n, mb, nb); A's block is mb for side L, nb for side R
SIZES = [(0, 0, 1, 1), (0, 2, 1, 2), (7, 0, 2, 1), (2, 2, 5, 5), (10, 10, 2, 3), (7, 7, 3, 2), (3, 2, 7, 7),
         (12, 3, 5, 5), (7, 6, 3, 2), (15, 7, 3, 5), (2, 3, 7, 7), (4, 13, 5, 5), (7, 8, 2, 9), (19, 25, 6, 5)]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def err_of(orc, t):
    return (8 if t in "cz" else 2) * orc.eps_of(orc.DTYPES[t])  # TypeUtilities<T>::error (util_types.h:40)


def alpha_of(dt, t):
    return dt(complex(-1.2, .7)) if t in "cz" else dt(-1.2)


def op_of(a, uplo, op, diag):
    """op(tri(A)) in extended precision: the referenced triangle, a unit diagonal for diag U"""
    wide = np.complex128 if a.dtype.kind == "c" else np.float64
    tri = np.tril(a) if uplo == "L" else np.triu(a)
    tri = tri.astype(wide)
    if diag == "U":
        np.fill_diagonal(tri, 1)
    return tri if op == "N" else tri.T if op == "T" else tri.conj().T


def random_case(rng, t, dt, side, uplo, diag, m, n):
    cx = t in "cz"
    na = m if side == "L" else n

    def rnd(r, c):
        return rng.uniform(-1, 1, (r, c)) + (1j * rng.uniform(-1, 1, (r, c)) if cx else 0)
    a = np.asfortranarray(rnd(na, na).astype(dt))
    # the entries outside the referenced triangle (and a unit diagonal) must not be read
    mask = np.triu(np.ones((na, na), bool), 1) if uplo == "L" else np.tril(np.ones((na, na), bool), -1)
    if diag == "U":
        mask |= np.eye(na, dtype=bool)
    a[mask] = -9.9
    return a, np.asfortranarray(rnd(m, n).astype(dt))


def check_product(a, b0, got, t, side, uplo, op, diag, alpha, tag):
    oa = op_of(a, uplo, op, diag)
    wb = b0.astype(oa.dtype)
    ref = alpha * (oa @ wb if side == "L" else wb @ oa)
    bound = abs(alpha) * (np.abs(oa) @ np.abs(wb) if side == "L" else np.abs(wb) @ np.abs(oa))
    k = oa.shape[0]
    eps = np.finfo(b0.real.dtype).eps
    err = np.abs(got.astype(oa.dtype) - ref)
    assert (err <= 8 * (k + 2) * eps * bound + 1e-30).all(), (tag, float((err / (bound + 1e-300)).max() / eps))


@pytest.mark.parametrize("t", TYPES)
def test_triangular_multiplication_analytic(dlaf, grid, oracle, t):
    dt = oracle.DTYPES[t]
    alpha = alpha_of(dt, t)
    for (m, n, mb, nb), (side, uplo, op, diag) in itertools.product(SIZES, VARIANTS):
        # op(A) X = B / alpha  <=>  B = alpha op(A) X
        a, b, x = oracle.triangular_system(side, uplo, op, diag, 1 / alpha, m, n, dt)
        nba = mb if side == "L" else nb
        # padded leading dimensions with sentinels, as a caller's ScaLAPACK-style local arrays have
        sa = np.full((a.shape[0] + 3, max(1, a.shape[1])), 5.5, dtype=dt, order="F")
        sb = np.full((m + 2, max(1, n)), 6.5, dtype=dt, order="F")
        sa[:a.shape[0], :a.shape[1]] = a
        sb[:m, :n] = x
        dlaf.triangular_multiplication(grid, side, uplo, op, diag, alpha, sa[:a.shape[0], :a.shape[1]], sb[:m, :n], nba,
                                       b_block=(mb, nb))
        tol = 40 * (m + 1) * err_of(oracle, t)
        ok, md = oracle.check_near(b, sb[:m, :n], tol, tol)
        assert ok, (md, tol, m, n, mb, nb, side, uplo, op, diag)
        assert (sb[m:, :] == 6.5).all() and np.array_equal(sa[:a.shape[0], :a.shape[1]], a)
        assert (sa[a.shape[0]:, :] == 5.5).all()


# (m, n, nb): several tiles, several 64-column blocks of the TRMM kernel, ragged last tiles, nb = 64 / 128 / 256
RANDOM_SIZES = [(150, 70, 32), (130, 257, 64), (333, 129, 100), (200, 300, 128), (1030, 1100, 256)]


@pytest.mark.parametrize("t", TYPES)
def test_triangular_multiplication_random_multi_tile(dlaf, grid, oracle, t):
    dt = oracle.DTYPES[t]
    alpha = alpha_of(dt, t)
    rng = np.random.default_rng(11)
    for (m, n, nb), (side, uplo, op, diag) in itertools.product(RANDOM_SIZES, VARIANTS):
        if t in "sc" and (side, op, diag) not in (("L", "N", "N"), ("R", "C", "U"), ("L", "T", "U"), ("R", "N", "N")):
            continue   # a subset for the single precision types
        if t == "z" and m > 1000 and (op, diag) != ("N", "N") and (side, uplo, op, diag) != ("R", "U", "C", "U"):
            continue
        a, b0 = random_case(rng, t, dt, side, uplo, diag, m, n)
        a_in = a.copy(order="F")
        b = b0.copy(order="F")
        dlaf.triangular_multiplication(grid, side, uplo, op, diag, alpha, a, b, nb)
        check_product(a, b0, b, t, side, uplo, op, diag, alpha, (m, n, nb, side, uplo, op, diag))
        assert np.array_equal(a, a_in)


def test_triangular_multiplication_fp64_1024(dlaf, grid, oracle):
    """the fp64 fast path's shape: whole 1024 tiles, many 64-column blocks per tile, both sweep directions"""
    rng = np.random.default_rng(12)
    dt = np.float64
    for side, uplo, op, diag in (("L", "L", "N", "N"), ("R", "U", "N", "N"), ("L", "L", "C", "N"), ("R", "L", "T", "U")):
        a, b0 = random_case(rng, "d", dt, side, uplo, diag, 2048, 2048)
        b = b0.copy(order="F")
        dlaf.triangular_multiplication(grid, side, uplo, op, diag, 0.75, a, b, 1024)
        check_product(a, b0, b, "d", side, uplo, op, diag, 0.75, (side, uplo, op, diag))
        ms, fl = dlaf.multiplication_profile()
        assert ms > 0 and fl == 2048.0 ** 3


@pytest.mark.parametrize("t", ["d", "z"])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_triangular_multiplication_resident(dlaf, grid, oracle, t, uplo):
    """resident operands: the factor factorize() left in HBM times a resident general matrix.  L L^H (B = L^H,
    side L, op N) / U^H U (B = U, side L, op C) must give back the SPD input to the Cholesky residual bound; and a
    general product against the extended-precision one."""
    dt = oracle.DTYPES[t]
    n, nb = 520, 128
    a0 = np.asfortranarray(oracle.set_random_hpd(n, nb, dt))
    A = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    A.upload(a0)
    assert A.factorize() == 0
    f = np.zeros((n, n), dtype=dt, order="F")
    A.download(f)
    fac = np.tril(f) if uplo == "L" else np.triu(f)
    Bd = dlaf.GeneralDeviceMatrix(grid, dt, n, n, nb)
    Bd.upload(np.asfortranarray(fac.conj().T if uplo == "L" else fac))
    dlaf.triangular_multiplication_device("L", uplo, "N" if uplo == "L" else "C", "N", dt(1), A, Bd)
    got = np.zeros((n, n), dtype=dt, order="F")
    Bd.download(got)
    eps = np.finfo(np.float64).eps
    assert np.abs(got - a0).max() <= 16 * n * eps * np.abs(a0).max(), np.abs(got - a0).max()
    # a general product on the resident factor: B = alpha B op(L) for a random B
    rng = np.random.default_rng(13)
    m = 300
    b0 = np.asfortranarray((rng.uniform(-1, 1, (m, n)) + (1j * rng.uniform(-1, 1, (m, n)) if t == "z" else 0)).astype(dt))
    B2 = dlaf.GeneralDeviceMatrix(grid, dt, m, n, nb)
    B2.upload(b0)
    alpha = alpha_of(dt, t)
    dlaf.triangular_multiplication_device("R", uplo, "T", "N", alpha, A, B2)
    got2 = np.zeros((m, n), dtype=dt, order="F")
    B2.download(got2)
    check_product(fac, b0, got2, t, "R", uplo, "T", "N", alpha, ("resident", uplo))
    for h in (B2, Bd, A):
        h.close()


@pytest.mark.parametrize("t", ["d", "z"])
def test_pxtrmm_and_solve_back(dlaf, grid, oracle, t):
    """p?trmm with 9-int descriptors; multiplication followed by triangular_solver with the same side / uplo / op / diag
    and 1 / alpha (op(A) X = B / alpha) returns B"""
    dt = oracle.DTYPES[t]
    rng = np.random.default_rng(14)
    alpha = alpha_of(dt, t)
    for (m, n, nb), (side, uplo, op, diag) in itertools.product([(150, 70, 32), (64, 200, 64)], VARIANTS):
        na = m if side == "L" else n
        a, b0 = random_case(rng, t, dt, side, uplo, diag, m, n)
        a[np.arange(na), np.arange(na)] = (a[np.arange(na), np.arange(na)] / na + 2) if diag == "N" else -9.9
        off = ~np.eye(na, dtype=bool) & (np.tril(np.ones((na, na), bool), -1) if uplo == "L" else np.triu(np.ones((na, na), bool), 1))
        a[off] /= na
        b = b0.copy(order="F")
        dlaf.pxtrmm(side, uplo, op, diag, m, n, alpha, a, 1, 1, [1, grid.context, na, na, nb, nb, 0, 0, max(1, na)],
                    b, 1, 1, [1, grid.context, m, n, nb, nb, 0, 0, max(1, m)])
        check_product(a, b0, b, t, side, uplo, op, diag, alpha, ("pxtrmm", m, n, side, uplo, op, diag))
        dlaf.triangular_solver(grid, side, uplo, op, diag, 1 / alpha, a, b, nb)
        scale = np.abs(b0).max()
        assert np.abs(b - b0).max() <= 50 * max(m, n) * np.finfo(b0.real.dtype).eps * scale, (m, n, side, uplo, op, diag)


def test_miniapp_triangular_multiplication():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_cpp_api
    exe = test_cpp_api.build_miniapp(name="miniapp_triangular_multiplication")
    r = subprocess.run([exe, "--m", "1500", "--n", "700", "--mb", "128", "--nb", "128", "--side", "L", "--uplo", "L",
                        "--op", "N", "--nruns", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s dLLNN \(1500, 700\) \(128, 128\) \(1, 1\) 1 GPU", r.stdout,
                          flags=re.M)) == 2, r.stdout
    resid = float(re.search(r"Solve-back residual max \|X - B\| / max \|B\| \(rank 0\): ([0-9.e+-]+)", r.stdout).group(1))
    assert resid < 1e-12, r.stdout


def launch_trmm_workers(nprow, npcol, order="R", timeout=600):
    from conftest import gpu_process_budget
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed import free_port
    n = nprow * npcol
    gpu_process_budget(n)
    port = str(free_port())
    procs = []
    for rank in range(n):
        env = dict(os.environ, OMP_NUM_THREADS="1", DLAF_MI355X_DEVICE="0", RANK=str(rank), WORLD_SIZE=str(n),
                   LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "trmm_dist_worker.py"), str(nprow),
                                       str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    rc = [p.returncode for p in procs]
    assert all(r == 0 for r in rc) and "TRMM_WORKER_RESULT OK" in outs[0][0], \
        (rc, outs[0][0][-2000:], "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
def test_triangular_multiplication_grid_2x3():
    launch_trmm_workers(2, 3)


# fresh_parent: the worker processes run about ten times slower once this pytest process has done GPU work of its own
# (conftest.py), which puts the 2 x 2 grid past its time limit when it runs behind the in-process tests of this file
@pytest.mark.fresh_parent
@pytest.mark.parametrize("nprow,npcol", [(1, 2), (2, 2)])
def test_triangular_multiplication_grid(nprow, npcol):
    launch_trmm_workers(nprow, npcol)
