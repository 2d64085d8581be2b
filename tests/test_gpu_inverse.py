"""triangular_inverse (xTRTRI) and inverse_from_cholesky_factor (xPOTRI) on the GPU against wide-precision numpy
references kept in this file: float64 / complex128 for s / c, longdouble / clongdouble for d / z.

Bounds (componentwise, n = order, eps = unit roundoff spacing of the working precision):
  triangular inverse      |W - W_ref| <= c n eps (|W_ref| |T| |W_ref|)                 (Higham's forward bound)
  inverse from factor     |X A - I|   <= c n eps (|W_ref|^H |W_ref| |L| |L|^H)         (upper: |W||W|^H |U|^H|U|)
                          ||I - A X||_1 / (n eps ||A||_1 ||X||_1) <= c                  (LAPACK xPOT03)
The constants c are 4 x the worst ratio the working-precision numpy / LAPACK route (np.linalg.inv of the triangle,
inv(L)^H inv(L)) reaches on the same inputs over every shape and variant below, and not below 1 (the margin: MFMA block
accumulation orders the sums differently from LAPACK).  Measured reference ratios (this file's calibrate(), x86-64,
numpy's OpenBLAS), per type [triangular inverse, componentwise product, xPOT03]:
    s, c  [0.1746, 0.3090, 0.3090]        d, z  [0.0557, 0.3384, 0.3384]
(each worst case is the 1 x 1 matrix, where n eps bounds a single rounding; at n >= 37 every ratio is below 0.06), so
c = 1 for the triangular inverse, 1.236 (s, c) and 1.354 (d, z) for the two checks of the product.

The single-precision types leave out the shapes (1030, 256) and (1100, 1024) (as the triangular multiplication's tests
do for their larger shapes); (1100, 1024) runs for d only.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
WIDE = {"s": np.float64, "d": np.longdouble, "c": np.complex128, "z": np.clongdouble}
EDGE = [(0, 4), (1, 4), (37, 64), (64, 64), (65, 64)]
TILE = [(130, 64), (192, 192), (200, 128), (333, 100)]
MULTI = [(600, 256), (1030, 256)]
SENTINEL = -9.9
PAD = 3
# 4 x the reference route's worst ratio, not below 1: [triangular inverse, componentwise product, xPOT03]
REF_RATIO = {"s": [0.1746, 0.3090, 0.3090], "d": [0.0557, 0.3384, 0.3384], "c": [0.1746, 0.3090, 0.3090],
             "z": [0.0557, 0.3384, 0.3384]}
C = {t: [max(1.0, 4 * r) for r in v] for t, v in REF_RATIO.items()}


def shapes_of(t):
    s = EDGE + TILE + [MULTI[0]]
    if t in "dz":
        s = s + [MULTI[1]]
    if t == "d":
        s = s + [(1100, 1024)]
    return s


CASES = [(t, n, nb) for t in "sdcz" for (n, nb) in shapes_of(t)]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def wide_tri_inv(t):
    """inverse of a lower triangular matrix in its own (wide) precision, by halves (numpy has no longdouble LAPACK)"""
    n = t.shape[0]
    if n <= 32:
        w = np.zeros_like(t)
        for j in range(n):
            w[j, j] = 1 / t[j, j]
            for i in range(j + 1, n):
                w[i, j] = -(t[i, j:i] @ w[j:i, j]) / t[i, i]
        return w
    h = n // 2
    a, b = wide_tri_inv(t[:h, :h]), wide_tri_inv(t[h:, h:])
    w = np.zeros_like(t)
    w[:h, :h], w[h:, h:] = a, b
    w[h:, :h] = -b @ (t[h:, :h] @ a)
    return w


@functools.lru_cache(maxsize=None)
def factor_of(t, n, seed=7):
    """the lower Cholesky factor (float64 / complex128, then cast) of a random Hermitian matrix plus n I"""
    rng = np.random.default_rng(seed + n)
    m = rng.uniform(-1, 1, (n, n)) + (1j * rng.uniform(-1, 1, (n, n)) if t in "cz" else 0)
    h = (m + m.conj().T) / 2 + n * np.eye(n)
    low = np.linalg.cholesky(h) if n else h
    low = low.astype(DT[t])
    low.setflags(write=False)
    return low


@functools.lru_cache(maxsize=None)
def lower_reference(t, n, diag):
    low = factor_of(t, n).astype(WIDE[t])
    if diag == "U" and n:
        low = np.tril(low, -1) / n + np.eye(n, dtype=WIDE[t])
        low = low.astype(DT[t]).astype(WIDE[t])  # the strict triangle as it is stored
    w = wide_tri_inv(low) if n else low
    low.setflags(write=False)
    w.setflags(write=False)
    return low, w


def reference(t, n, uplo, diag):
    """(T, W_ref) in the wide precision: the operand as the device sees it and its inverse (computed once per t, n,
    diag; the upper case is its adjoint)"""
    low, w = lower_reference(t, n, diag)
    return (low, w) if uplo == "L" else (low.conj().T, w.conj().T)


def padded(t, tri, uplo, diag):
    """the stored operand: padded leading dimension, sentinels outside the referenced triangle (diag U: on it too)"""
    n = tri.shape[0]
    buf = np.full((n + PAD, n), SENTINEL, dtype=DT[t], order="F")
    a = buf[:n, :]
    mask = np.tril(np.ones((n, n), bool)) if uplo == "L" else np.triu(np.ones((n, n), bool))
    if diag == "U":
        mask &= ~np.eye(n, dtype=bool)
    a[mask] = tri.astype(DT[t])[mask]
    return buf, a, mask


def same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def untouched(buf, buf0, mask):
    n = mask.shape[0]
    outside = np.ones(buf.shape, bool)
    outside[:n, :][mask] = False
    return np.array_equal(buf[outside].view(np.uint8), buf0[outside].view(np.uint8))


def trtri_ratio(t, got, tri, wref, mask):
    n = tri.shape[0]
    if not mask.any():
        return 0.0
    eps = np.finfo(DT[t]).eps
    aw, at = np.abs(wref).astype(np.float64), np.abs(tri).astype(np.float64)
    bound = aw @ at @ aw  # (a sum of non-negative terms: float64 carries it to 1e-13 of itself)
    err = np.abs(got.astype(WIDE[t]) - wref).astype(np.float64)
    return float((err[mask] / (n * eps * bound[mask])).max())


def potri_ratios(t, got_tri, tri, wref, uplo):
    """got_tri: the returned triangle (anything outside it ignored)"""
    n = tri.shape[0]
    if n == 0:
        return 0.0, 0.0
    eps = np.finfo(DT[t]).eps
    g = got_tri.astype(WIDE[t])
    x = np.tril(g) + np.tril(g, -1).conj().T if uplo == "L" else np.triu(g) + np.triu(g, 1).conj().T
    a = tri @ tri.conj().T if uplo == "L" else tri.conj().T @ tri
    aw, at = np.abs(wref).astype(np.float64), np.abs(tri).astype(np.float64)
    bound = (aw.T @ aw) @ (at @ at.T) if uplo == "L" else (aw @ aw.T) @ (at.T @ at)
    res = x @ a - np.eye(n, dtype=WIDE[t])
    comp = float((np.abs(res).astype(np.float64) / (n * eps * bound)).max())
    one = lambda m: float(np.abs(m).sum(axis=0).max())
    # A and X are Hermitian: I - A X = (I - X A)^H, no second wide product
    pot03 = one(res.conj().T) / (n * eps * one(a) * one(x))
    return comp, pot03


def calibrate():
    """the reference route's ratios (module docstring): np.linalg.inv of the triangle and inv(L)^H inv(L) in the working
    precision, on every input of this file"""
    worst = {t: [0.0, 0.0, 0.0] for t in "sdcz"}
    for (t, n, nb) in CASES:
        if n == 0:
            continue
        for uplo in "LU":
            for diag in "NU":
                tri, wref = reference(t, n, uplo, diag)
                mask = padded(t, tri, uplo, diag)[2] | np.eye(n, dtype=bool)
                w = np.linalg.inv(tri.astype(DT[t]))
                worst[t][0] = max(worst[t][0], trtri_ratio(t, w, tri, wref, mask))
            tri, wref = reference(t, n, uplo, "N")
            w = np.linalg.inv(tri.astype(DT[t]))
            x = w.conj().T @ w if uplo == "L" else w @ w.conj().T
            comp, p3 = potri_ratios(t, x, tri, wref, uplo)
            worst[t][1] = max(worst[t][1], comp)
            worst[t][2] = max(worst[t][2], p3)
        print(t, n, worst[t], flush=True)
    return worst


@pytest.mark.parametrize("diag", "NU")
@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("t,n,nb", CASES)
def test_triangular_inverse(dlaf, grid, t, n, nb, uplo, diag):
    tri, wref = reference(t, n, uplo, diag)
    buf, a, mask = padded(t, tri, uplo, diag)
    buf0 = buf.copy()
    assert dlaf.triangular_inverse(grid, uplo, diag, a, nb, n=n) == 0
    assert untouched(buf, buf0, mask)
    r = trtri_ratio(t, a, tri, wref, mask)
    print(f"triangular_inverse {t} n={n} nb={nb} {uplo}{diag}: ratio {r:.4f} (c = {C[t][0]})")
    assert r <= C[t][0]


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("t,n,nb", CASES)
def test_inverse_from_cholesky_factor(dlaf, grid, t, n, nb, uplo):
    tri, wref = reference(t, n, uplo, "N")
    buf, a, mask = padded(t, tri, uplo, "N")
    buf0 = buf.copy()
    assert dlaf.inverse_from_cholesky_factor(grid, uplo, a, nb, n=n) == 0
    assert untouched(buf, buf0, mask)
    if t in "cz":
        assert (np.diagonal(a).imag == 0).all()
    comp, p3 = potri_ratios(t, a, tri, wref, uplo)
    print(f"inverse_from_cholesky_factor {t} n={n} nb={nb} {uplo}: ratios {comp:.4f} {p3:.4f} (c = {C[t][1:]})")
    assert comp <= C[t][1] and p3 <= C[t][2]


@pytest.mark.parametrize("t,uplo", [("d", "L"), ("z", "U"), ("s", "U"), ("c", "L")])
def test_resident_factor_matches_potrs_against_identity(dlaf, grid, t, uplo):
    """potrf -> invert_from_factor on a resident matrix against potrs_device with the identity, both held to the bound"""
    n, nb = 333, 100
    low = factor_of(t, n).astype(WIDE[t])
    h = (low @ low.conj().T).astype(DT[t])
    m = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    m.upload(np.asfortranarray(h))
    assert m.factorize() == 0
    fac = np.zeros((n, n), DT[t], order="F")
    m.download(fac)
    b = dlaf.GeneralDeviceMatrix(grid, DT[t], n, n, nb)
    b.upload(np.asfortranarray(np.eye(n, dtype=DT[t])))
    dlaf.potrs_device(uplo, m, b)
    via_solve = np.zeros((n, n), DT[t], order="F")
    b.download(via_solve)
    assert m.invert_from_factor() == 0
    got = np.zeros((n, n), DT[t], order="F")
    m.download(got)
    tri = (np.tril(fac) if uplo == "L" else np.triu(fac)).astype(WIDE[t])
    lw = wide_tri_inv(tri if uplo == "L" else tri.conj().T)
    wref = lw if uplo == "L" else lw.conj().T
    for name, x in (("invert_from_factor", got), ("potrs_device", via_solve)):
        comp, p3 = potri_ratios(t, x, tri, wref, uplo)
        print(f"{name} {t} {uplo}: ratios {comp:.4f} {p3:.4f}")
        assert comp <= C[t][1] and p3 <= C[t][2], name
    if t in "cz":
        assert (np.diagonal(got).imag == 0).all()


@pytest.mark.parametrize("t,uplo,diag", [("d", "L", "N"), ("z", "U", "U"), ("s", "U", "N"), ("c", "L", "U")])
def test_inverse_times_original_is_identity(dlaf, grid, t, uplo, diag):
    """triangular_inverse, then triangular_multiplication with the original: the identity within the TRMM tests' bound
    8 (k + 2) eps |T| |W| on top of the inverse's own c n eps |T| |W_ref| |T| |W_ref|"""
    n, nb = 200, 128
    tri, wref = reference(t, n, uplo, diag)
    _, a, _ = padded(t, tri, uplo, diag)
    orig = np.asfortranarray(a.copy())
    assert dlaf.triangular_inverse(grid, uplo, diag, a, nb, n=n) == 0
    w = np.tril(a) if uplo == "L" else np.triu(a)
    if diag == "U":
        np.fill_diagonal(w, 1)
    b = np.asfortranarray(w.astype(DT[t]))
    dlaf.triangular_multiplication(grid, "L", uplo, "N", diag, DT[t](1), orig, b, nb)
    eps = np.finfo(DT[t]).eps
    at, aw = np.abs(tri).astype(np.float64), np.abs(wref).astype(np.float64)
    bound = 8 * (n + 2) * eps * (at @ aw) + C[t][0] * n * eps * (at @ aw @ at @ aw)
    err = np.abs(b.astype(WIDE[t]) - np.eye(n)).astype(np.float64)
    assert (err <= bound).all(), float((err / bound).max())


INFO_CASES = [("first", [0]), ("tile boundary", [256]), ("ragged last tile", [590]), ("two zeros", [300, 101])]


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("t", "dz")
@pytest.mark.parametrize("name,where", INFO_CASES)
def test_info_and_untouched_operand(dlaf, grid, name, where, t, uplo):
    n, nb = 600, 256
    tri, _ = reference(t, n, uplo, "N")
    buf, a, _ = padded(t, tri, uplo, "N")
    for i in where:
        a[i, i] = 0
    buf0 = buf.copy()
    assert dlaf.triangular_inverse(grid, uplo, "N", a, nb, n=n) == min(where) + 1
    assert same_bits(buf, buf0)
    assert dlaf.inverse_from_cholesky_factor(grid, uplo, a, nb, n=n) == min(where) + 1
    assert same_bits(buf, buf0)
    m = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    m.upload(np.asfortranarray(a))
    assert m.invert_triangular("N") == min(where) + 1
    back = np.asfortranarray(a.copy())
    m.download(back)
    assert same_bits(back, a)


def test_unit_diagonal_ignores_a_stored_zero(dlaf, grid):
    n, nb = 130, 64
    tri, wref = reference("d", n, "L", "U")
    buf, a, mask = padded("d", tri, "L", "U")
    np.fill_diagonal(a, 0)
    buf0 = buf.copy()
    assert dlaf.triangular_inverse(grid, "L", "U", a, nb, n=n) == 0
    assert untouched(buf, buf0, mask)
    assert trtri_ratio("d", a, tri, wref, mask) <= C["d"][0]


@pytest.mark.parametrize("t,uplo", [("d", "U"), ("c", "L")])
def test_scalapack_entries_and_resident_operands(dlaf, grid, t, uplo):
    n, nb = 130, 64
    tri, wref = reference(t, n, uplo, "N")
    desc = [1, grid.context, n, n, nb, nb, 0, 0, n + PAD]
    buf, a, mask = padded(t, tri, uplo, "N")
    assert dlaf.pxtrtri(uplo, "N", n, a, 1, 1, desc) == 0
    assert trtri_ratio(t, a, tri, wref, mask) <= C[t][0]
    buf, a, mask = padded(t, tri, uplo, "N")
    assert dlaf.pxpotri(uplo, n, a, 1, 1, desc) == 0
    comp, p3 = potri_ratios(t, a, tri, wref, uplo)
    assert comp <= C[t][1] and p3 <= C[t][2]
    # resident
    _, a, mask = padded(t, tri, uplo, "N")
    m = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    m.upload(np.asfortranarray(a))
    assert m.invert_triangular("N") == 0
    got = np.asfortranarray(a.copy())
    m.download(got)
    assert trtri_ratio(t, got, tri, wref, mask) <= C[t][0]
    m.upload(np.asfortranarray(a))
    assert m.invert_from_factor() == 0
    m.download(got)
    comp, p3 = potri_ratios(t, got, tri, wref, uplo)
    assert comp <= C[t][1] and p3 <= C[t][2]


@pytest.mark.parametrize("t", "dz")
def test_inverse_profile(dlaf, grid, t):
    n, nb = 600, 256
    tri, _ = reference(t, n, "L", "N")
    cx = 4.0 if t == "z" else 1.0
    _, a, _ = padded(t, tri, "L", "N")
    assert dlaf.triangular_inverse(grid, "L", "N", a, nb, n=n) == 0
    ms, flops = dlaf.inverse_profile()
    assert ms > 0 and flops == pytest.approx(cx * n ** 3 / 3)
    _, a, _ = padded(t, tri, "L", "N")
    assert dlaf.inverse_from_cholesky_factor(grid, "L", a, nb, n=n) == 0
    ms, flops = dlaf.inverse_profile()
    assert ms > 0 and flops == pytest.approx(2 * cx * n ** 3 / 3)


def test_miniapp_checks_its_result():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import test_cpp_api
    exe = test_cpp_api.build_miniapp(name="miniapp_inverse_from_cholesky_factor")
    r = subprocess.run([exe, "--matrix-size", "600", "--block-size", "256", "--nruns", "2", "--check-result", "last"],
                       cwd=root, capture_output=True, text=True, timeout=300, env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s dL \(600, 600\) \(256, 256\) \(1, 1\) 1 GPU", r.stdout,
                          flags=re.M)) == 2, r.stdout
    assert len(re.findall(r"^Check: .* PASSED$", r.stdout, flags=re.M)) == 1, r.stdout
