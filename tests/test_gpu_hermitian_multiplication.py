"""Hermitian multiplication on the GPU: C = beta C + alpha A B / beta C + alpha B A against the reference's known-answer
system (test/include/dlaf_test/matrix/util_generic_blas.h getHermitianMatrixMultiplication, restated below, at the
reference's own sizes and tolerance), against float64 / complex128 products of random operands on multi-tile shapes,
with beta = 0 over a C full of NaN, with a complex diagonal, on resident operands, through p?symm / p?hemm, in the
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
VARIANTS = list(itertools.product("LR", "LU"))
# test_multiplication_hermitian.cpp: (m, n, mb, nb); A's block is mb for side L, nb for side R
SIZES = [(0, 0, 1, 1), (0, 2, 1, 2), (7, 0, 2, 1), (2, 2, 5, 5), (10, 10, 2, 3), (7, 7, 3, 2), (3, 2, 7, 7),
         (12, 3, 5, 5), (7, 6, 3, 2), (15, 7, 3, 5), (2, 3, 7, 7), (4, 13, 5, 5), (7, 8, 2, 9), (19, 25, 6, 5)]
GAMMA = float(np.float32(1.3))


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def err_of(t):
    return (8 if t in "cz" else 2) * float(np.finfo(DT[t]).eps)  # TypeUtilities<T>::error (util_types.h:40)


DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def scalars(t):
    dt = DT[t]
    return (dt(complex(-1.2, .7)), dt(complex(1.12, -.1))) if t in "cz" else (dt(-1.2), dt(1.12))


def hermitian_system(side, uplo, m, n, alpha, beta, dt):
    """getHermitianMatrixMultiplication: (A, B, C, result).  polar(r, theta) is r for real types.
    A(row, col) = .9 (row+1)(col+1) e^{i gamma (row - col)} for side L and e^{i gamma (col - row)} for side R (with the
    other sign the closed form does not hold), (-99, -87) outside the uplo triangle;
    B(r, c) = .7 / ((r+1)(c+1)) e^{i gamma (r + c)};  C(i, j) = 1.2 i / (j+1) e^{i (j - i)};
    result = beta C + .63 k alpha (i+1)/(j+1) [L] or (j+1)/(i+1) [R] e^{i gamma (i + j)}, k = A's size."""
    cx = np.dtype(dt).kind == "c"
    k = m if side == "L" else n

    def polar(r, th):
        return r * np.exp(1j * th) if cx else r + 0 * th
    r_ = np.arange(k, dtype=np.float64)[:, None]
    c_ = np.arange(k, dtype=np.float64)[None, :]
    a = polar(.9 * (r_ + 1) * (c_ + 1), GAMMA * ((r_ - c_) if side == "L" else (c_ - r_)))
    skip = (r_ < c_) if uplo == "L" else (r_ > c_)
    a = np.where(skip, complex(-99, -87) if cx else -99.0, a)
    i = np.arange(m, dtype=np.float64)[:, None]
    j = np.arange(n, dtype=np.float64)[None, :]
    b = polar(.7 / ((i + 1) * (j + 1)), GAMMA * (i + j))
    c = polar(1.2 * i / (j + 1), j - i)
    wide = np.complex128 if cx else np.float64
    res = wide(beta) * c + .63 * k * wide(alpha) * polar((i + 1) / (j + 1) if side == "L" else (j + 1) / (i + 1),
                                                          GAMMA * (i + j))
    f = np.asfortranarray
    return f(a.astype(dt)), f(b.astype(dt)), f(c.astype(dt)), f(res.astype(dt))


def check_near(expected, actual, rel, abs_):
    """CHECK_MATRIX_NEAR (test/include/dlaf_test/matrix/util_matrix.h): diff < abs OR diff / max(|e|, |a|) < rel"""
    diff = np.abs(expected - actual)
    big = np.maximum(np.abs(expected), np.abs(actual))
    with np.errstate(divide="ignore", invalid="ignore"):
        relok = np.where(big > 0, diff / np.where(big > 0, big, 1), np.inf) < rel
    return bool(((diff < abs_) | relok).all()), (float(diff.max()) if diff.size else 0.0)


def padded(x, extra, sentinel):
    s = np.full((x.shape[0] + extra, max(1, x.shape[1])), sentinel, dtype=x.dtype, order="F")
    s[:x.shape[0], :x.shape[1]] = x
    return s


@pytest.mark.parametrize("t", TYPES)
def test_hermitian_multiplication_analytic(dlaf, grid, t):
    dt = DT[t]
    alpha, beta = scalars(t)
    for (m, n, mb, nb), (side, uplo) in itertools.product(SIZES, VARIANTS):
        a, b, c, res = hermitian_system(side, uplo, m, n, alpha, beta, dt)
        na = a.shape[0]
        # padded leading dimensions with sentinels, as a caller's ScaLAPACK-style local arrays have
        sa, sb, sc = padded(a, 3, 5.5), padded(b, 2, 6.5), padded(c, 1, 7.5)
        dlaf.hermitian_multiplication(grid, side, uplo, alpha, sa[:na, :na], sb[:m, :n], beta, sc[:m, :n],
                                      mb if side == "L" else nb, c_block=(mb, nb))
        tol = 10 * (m + 1) * err_of(t)
        ok, md = check_near(res, sc[:m, :n], tol, tol)
        print(f"analytic {t} {side}{uplo} {m}x{n} ({mb},{nb}): max diff {md:.3e} tol {tol:.3e}")
        assert ok, (md, tol, m, n, mb, nb, side, uplo)
        assert (sc[m:, :] == 7.5).all() and (sb[m:, :] == 6.5).all() and (sa[na:, :] == 5.5).all()
        assert np.array_equal(sa[:na, :na], a) and np.array_equal(sb[:m, :n], b)


def random_case(rng, t, side, uplo, m, n, sentinel=np.nan):
    dt = DT[t]
    cx = t in "cz"
    na = m if side == "L" else n

    def rnd(r, c):
        return np.asfortranarray((rng.uniform(-1, 1, (r, c)) + (1j * rng.uniform(-1, 1, (r, c)) if cx else 0)).astype(dt))
    a = rnd(na, na)
    a[np.arange(na), np.arange(na)] = a[np.arange(na), np.arange(na)].real
    # the other triangle must not be read
    a[np.triu(np.ones((na, na), bool), 1) if uplo == "L" else np.tril(np.ones((na, na), bool), -1)] = sentinel
    return a, rnd(m, n), rnd(m, n)


def herm_image(a, uplo):
    """the Hermitian matrix whose uplo triangle is stored in a (real diagonal), in extended precision"""
    wide = np.complex128 if a.dtype.kind == "c" else np.float64
    tri = (np.tril(a, -1) if uplo == "L" else np.triu(a, 1)).astype(wide)
    return tri + tri.conj().T + np.diag(np.diag(a).real.astype(wide))


def check_product(a, b, c0, got, side, uplo, alpha, beta, tag):
    """componentwise forward bound of a length-na dot product, c = 8 as check_product of the triangular multiplication's
    tests: |got - ref| <= 8 (na + 2) eps (|beta| |C0| + |alpha| |A| |B|)"""
    h = herm_image(a, uplo)
    wb, wc = b.astype(h.dtype), c0.astype(h.dtype)
    al, be = h.dtype.type(alpha), h.dtype.type(beta)
    ref = be * wc + al * (h @ wb if side == "L" else wb @ h)
    bound = abs(be) * np.abs(wc) + abs(al) * (np.abs(h) @ np.abs(wb) if side == "L" else np.abs(wb) @ np.abs(h))
    eps = np.finfo(c0.real.dtype).eps
    err = np.abs(got.astype(h.dtype) - ref)
    assert np.isfinite(got).all(), tag
    worst = float((err / (bound + 1e-300)).max() / eps)
    print(f"product {tag}: worst err / (eps bound) = {worst:.3f} of {8 * (h.shape[0] + 2)}")
    assert (err <= 8 * (h.shape[0] + 2) * eps * bound + 1e-30).all(), (tag, worst)


# (m, n, nb of A, free block): several tiles, several 128-blocks per tile, ragged last tiles in both dimensions,
# nb = 32 / 64 / 100 / 128 / 256, MB != NB in the free dimension
RANDOM_SIZES = [(150, 70, 32, 32), (130, 257, 64, 64), (333, 129, 100, 100), (200, 300, 128, 128), (1030, 1100, 256, 256),
                (150, 170, 32, 48), (300, 260, 128, 100)]


@pytest.mark.parametrize("t", TYPES)
def test_hermitian_multiplication_random_multi_tile(dlaf, grid, t):
    alpha, beta = scalars(t)
    rng = np.random.default_rng(21)
    for (m, n, nb, nbf), (side, uplo) in itertools.product(RANDOM_SIZES, VARIANTS):
        if t in "sc" and m > 1000 and (side, uplo) not in (("L", "U"), ("R", "L")):
            continue   # the single precision types run two of the four variants at the largest shape
        a, b, c0 = random_case(rng, t, side, uplo, m, n)
        a_in, b_in = a.copy(order="F"), b.copy(order="F")
        c = c0.copy(order="F")
        dlaf.hermitian_multiplication(grid, side, uplo, alpha, a, b, beta, c, nb,
                                      c_block=(nb, nbf) if side == "L" else (nbf, nb))
        check_product(a, b, c0, c, side, uplo, alpha, beta, (t, m, n, nb, nbf, side, uplo))
        assert np.array_equal(a, a_in, equal_nan=True) and np.array_equal(b, b_in)


def test_hermitian_multiplication_fp64_1024(dlaf, grid):
    """the fp64 fast path's shape: whole 1024 tiles, the vector loaders of all three fetch modes"""
    rng = np.random.default_rng(22)
    for side, uplo in VARIANTS:
        a, b, c0 = random_case(rng, "d", side, uplo, 2048, 2048)
        c = c0.copy(order="F")
        dlaf.hermitian_multiplication(grid, side, uplo, 0.75, a, b, -0.5, c, 1024)
        check_product(a, b, c0, c, side, uplo, 0.75, -0.5, ("fp64_1024", side, uplo))
        ms, fl = dlaf.multiplication_profile()
        assert ms > 0 and fl == 2 * 2048.0 ** 3


@pytest.mark.parametrize("t", TYPES)
def test_hermitian_multiplication_beta_zero_nan(dlaf, grid, t):
    """beta = 0: C is not read -- a C full of NaN gives the finite alpha A B"""
    alpha, _ = scalars(t)
    rng = np.random.default_rng(23)
    for (m, n, nb), (side, uplo) in itertools.product([(150, 70, 32), (260, 300, 128)], VARIANTS):
        a, b, _ = random_case(rng, t, side, uplo, m, n)
        c = np.full((m, n), np.nan, dtype=DT[t], order="F")
        dlaf.hermitian_multiplication(grid, side, uplo, alpha, a, b, 0, c, nb)
        check_product(a, b, np.zeros((m, n), dtype=DT[t]), c, side, uplo, alpha, 0, ("beta0", t, m, n, side, uplo))


@pytest.mark.parametrize("t", ["c", "z"])
def test_hermitian_multiplication_complex_diagonal_ignored(dlaf, grid, t):
    """xHEMM semantics: the imaginary part of A's diagonal is not read"""
    alpha, beta = scalars(t)
    rng = np.random.default_rng(24)
    for (m, n, nb), (side, uplo) in itertools.product([(150, 70, 32), (260, 300, 128)], VARIANTS):
        a, b, c0 = random_case(rng, t, side, uplo, m, n)
        na = a.shape[0]
        c1, c2 = c0.copy(order="F"), c0.copy(order="F")
        dlaf.hermitian_multiplication(grid, side, uplo, alpha, a, b, beta, c1, nb)
        a2 = a.copy(order="F")
        a2[np.arange(na), np.arange(na)] += 1j * rng.uniform(1, 2, na).astype(a.real.dtype)
        dlaf.hermitian_multiplication(grid, side, uplo, alpha, a2, b, beta, c2, nb)
        assert np.array_equal(c1, c2), (t, m, n, side, uplo)


@pytest.mark.parametrize("t", ["d", "z"])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_hermitian_multiplication_resident(dlaf, grid, oracle, t, uplo):
    """resident operands: only C changes; and with A SPD and factored on a copy, A B equals the two triangular
    multiplications L (L^H B) / U^H (U B) to the bound test_triangular_multiplication_resident uses for L L^H against A"""
    dt = DT[t]
    alpha, beta = scalars(t)
    rng = np.random.default_rng(25)
    n, nb = 520, 128
    for side, m2 in (("L", 300), ("R", 300)):
        mm, nn = (n, m2) if side == "L" else (m2, n)
        a, b, c0 = random_case(rng, t, side, uplo, mm, nn, sentinel=0)
        A = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
        A.upload(a)
        B = dlaf.GeneralDeviceMatrix(grid, dt, mm, nn, nb)
        Cm = dlaf.GeneralDeviceMatrix(grid, dt, mm, nn, nb)
        B.upload(b)
        Cm.upload(c0)
        dlaf.hermitian_multiplication_device(side, uplo, alpha, A, B, beta, Cm)
        got = np.zeros((mm, nn), dtype=dt, order="F")
        Cm.download(got)
        check_product(a, b, c0, got, side, uplo, alpha, beta, ("resident", t, side, uplo))
        fa = np.zeros((n, n), dtype=dt, order="F")
        A.download(fa)
        fb = np.zeros((mm, nn), dtype=dt, order="F")
        B.download(fb)
        tri = np.tril if uplo == "L" else np.triu
        assert np.array_equal(tri(fa), tri(a)) and np.array_equal(fb, b)
        for h in (Cm, B, A):
            h.close()
    # consistency with the triangular multiplication
    a0 = np.asfortranarray(oracle.set_random_hpd(n, nb, dt))
    A = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    F = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    A.upload(a0)
    F.upload(a0)
    assert F.factorize() == 0
    b = np.asfortranarray((rng.uniform(-1, 1, (n, 200)) + (1j * rng.uniform(-1, 1, (n, 200)) if t == "z" else 0)).astype(dt))
    B = dlaf.GeneralDeviceMatrix(grid, dt, n, 200, nb)
    Cm = dlaf.GeneralDeviceMatrix(grid, dt, n, 200, nb)
    T2 = dlaf.GeneralDeviceMatrix(grid, dt, n, 200, nb)
    B.upload(b)
    T2.upload(b)
    Cm.upload(np.full((n, 200), np.nan, dtype=dt, order="F"))
    dlaf.hermitian_multiplication_device("L", uplo, dt(1), A, B, dt(0), Cm)
    # A = L L^H: L (L^H B);  A = U^H U: U^H (U B)
    dlaf.triangular_multiplication_device("L", uplo, "C" if uplo == "L" else "N", "N", dt(1), F, T2)
    dlaf.triangular_multiplication_device("L", uplo, "N" if uplo == "L" else "C", "N", dt(1), F, T2)
    got = np.zeros((n, 200), dtype=dt, order="F")
    two = np.zeros((n, 200), dtype=dt, order="F")
    Cm.download(got)
    T2.download(two)
    eps = np.finfo(np.float64).eps
    diff = np.abs(got - two).max()
    print(f"resident consistency {t} {uplo}: max diff {diff:.3e} bound {16 * n * eps * np.abs(a0).max():.3e}")
    assert diff <= 16 * n * eps * np.abs(a0).max(), diff
    for h in (T2, Cm, B, F, A):
        h.close()


@pytest.mark.parametrize("t", ["d", "z"])
def test_pxhemm(dlaf, grid, t):
    """p?symm / p?hemm with 9-int descriptors"""
    alpha, beta = scalars(t)
    rng = np.random.default_rng(26)
    for (m, n, nb), (side, uplo) in itertools.product([(150, 70, 32), (64, 200, 64)], VARIANTS):
        na = m if side == "L" else n
        a, b, c0 = random_case(rng, t, side, uplo, m, n)
        c = c0.copy(order="F")
        dlaf.pxhemm(side, uplo, m, n, alpha, a, 1, 1, [1, grid.context, na, na, nb, nb, 0, 0, max(1, na)],
                    b, 1, 1, [1, grid.context, m, n, nb, nb, 0, 0, max(1, m)], beta,
                    c, 1, 1, [1, grid.context, m, n, nb, nb, 0, 0, max(1, m)])
        check_product(a, b, c0, c, side, uplo, alpha, beta, ("pxhemm", t, m, n, side, uplo))


def test_miniapp_hermitian_multiplication():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_cpp_api
    exe = test_cpp_api.build_miniapp(name="miniapp_hermitian_multiplication")
    r = subprocess.run([exe, "--m", "1500", "--n", "700", "--mb", "128", "--nb", "128", "--side", "L", "--uplo", "U",
                        "--type", "z", "--beta", "0.25", "--nruns", "2", "--check-result", "last"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s zLU \(1500, 700\) \(128, 128\) \(1, 1\) 1 GPU", r.stdout,
                          flags=re.M)) == 2, r.stdout
    resid = float(re.search(r"Check residual max \|C v - \(beta C_0 v \+ alpha A B v\)\| / max \|\.\| : ([0-9.e+-]+)",
                            r.stdout).group(1))
    assert resid < 1e-12, r.stdout


def launch_hemm_workers(nprow, npcol, order="R", timeout=600):
    from conftest import gpu_process_budget
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed import free_port
    n = nprow * npcol
    assert n <= 6
    gpu_process_budget(n)
    port = str(free_port())
    procs = []
    outs = []
    try:
        for rank in range(n):
            env = dict(os.environ, OMP_NUM_THREADS="1", DLAF_MI355X_DEVICE="0", RANK=str(rank), WORLD_SIZE=str(n),
                       LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "hemm_dist_worker.py"), str(nprow),
                                           str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True))
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    rc = [p.returncode for p in procs]
    assert all(r == 0 for r in rc) and "HEMM_WORKER_RESULT OK" in outs[0][0], \
        (rc, outs[0][0][-2000:], "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
def test_hermitian_multiplication_grid_2x3():
    launch_hemm_workers(2, 3)


# fresh_parent: the worker processes run about ten times slower once this pytest process has done GPU work of its own
# (conftest.py)
@pytest.mark.fresh_parent
@pytest.mark.parametrize("nprow,npcol", [(1, 2), (2, 2)])
def test_hermitian_multiplication_grid(nprow, npcol):
    launch_hemm_workers(nprow, npcol)
