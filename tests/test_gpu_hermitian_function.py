"""Functions of a Hermitian matrix on the GPU (hermitian_function, hermitian_power and their resident forms): the
eigensolver, one call of the weights callback, and the weighted rank-k update with the eigenvectors still in HBM.

Input: A = Q diag(lambda) Q^H with lambda = linspace(0.5, 8, n) and Q from a QR of a seeded Gaussian matrix.  Only the
lower triangle is passed; the other one is filled with -9.9 and must come back bit for bit.

Bound: max |f(A)_gpu - f(A)_ref| <= n u (max |f(lambda)| + L lambda_max), u the unit roundoff of the type and L the largest
|f'| on [0.5, 8]: the eigensolver's backward error (the project's n * error_of convention, relative to |A| = lambda_max)
carried through f's Lipschitz constant, plus the synthesis's own rounding against max |f|.  The reference is numpy's
eigh-based f(A) in the wide type.  numpy's own float32 / complex64 synthesis on these inputs stays at or below 0.03 of the
bound for n in {34, 150, 357}.

Ratios error / bound reached on an MI355X (one run; the tests print them): x^(1/2) is the largest everywhere -- 0.19 (d)
and 0.11 (z) at n = 34, nb = 8; 0.13 at (34, 13); 0.10 (s, c) and 0.03 (d, z) at n = 150; 0.015 at n = 357 -- the other
three functions stay between 0.001 and 0.04; hermitian_power(-1/2): 0.019 (s, c), 0.005 - 0.006 (d, z) at 150, 0.003 at
357; the pseudo-inverse above a threshold: 0.002 (d), 0.001 (z).  For d and z the reference's eigh runs in double (numpy's
linalg stops there) and only its synthesis in the wide type, so these ratios include the reference's own error."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
WIDE = {"s": np.float64, "d": np.longdouble, "c": np.complex128, "z": np.clongdouble}
LO, HI = 0.5, 8.0
# name -> (f, max |f| on [LO, HI], max |f'| on [LO, HI])
FUNCS = {
    "rsqrt": (lambda x: x ** -0.5, LO ** -0.5, 0.5 * LO ** -1.5),
    "sqrt": (lambda x: x ** 0.5, HI ** 0.5, 0.5 * LO ** -0.5),
    "inv": (lambda x: 1 / x, 1 / LO, LO ** -2),
    "exp": (lambda x: np.exp(-x), float(np.exp(-LO)), float(np.exp(-LO))),
}
# (n, nb, eigensolver_min_band): the eigensolver's own small sizes (test_gpu_eigensolver.py), n = 1, and two multi-block ones
SIZES = [(34, 8, 3), (34, 13, 100), (1, 4, 100), (150, 64, 100), (357, 160, 100)]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


@pytest.fixture
def min_band(dlaf):
    old = dlaf.eigensolver_min_band()
    yield dlaf.eigensolver_min_band
    dlaf.eigensolver_min_band(old)


_cache = {}


def matrix(t, n):
    """(A in the wide type, lambda, Q): computed once per (type, n) and never changed"""
    if (t, n) not in _cache:
        rng = np.random.default_rng(1000 + n)
        g = rng.standard_normal((n, n))
        if t in "cz":
            g = g + 1j * rng.standard_normal((n, n))
        q = np.linalg.qr(g)[0].astype(WIDE[t])  # (numpy's linalg stops at double: orthogonal to double roundoff)
        lam = np.linspace(LO, HI, n) if n > 1 else np.array([LO])
        a = (q * lam[None, :]) @ q.conj().T
        a = (a + a.conj().T) / 2
        for x in (a, lam, q):
            x.setflags(write=False)
        _cache[(t, n)] = (a, lam, q)
    return _cache[(t, n)]


def reference(t, n, g_of):
    """f(A) in the wide type from numpy's eigh of the ROUNDED input (what the GPU sees); g_of: eigenvalues -> weights"""
    a, _, _ = matrix(t, n)
    ar = a.astype(DT[t]).astype(WIDE[t])
    w, z = np.linalg.eigh(ar.astype(np.complex128 if t in "cz" else np.float64))
    z = z.astype(WIDE[t])
    return (z * g_of(w)[None, :].astype(WIDE[t])) @ z.conj().T, w


def lower_input(t, n):
    a, _, _ = matrix(t, n)
    x = np.asfortranarray(a.astype(DT[t]))
    x[np.triu_indices(n, 1)] = -9.9
    return x


def bound(t, n, fmax, lip):
    u = float(np.finfo(DT[t]).eps) / 2
    return n * u * (fmax + lip * HI)


def check_triangle(t, got, want, bnd, what):
    n = got.shape[0]
    up = np.triu_indices(n, 1)
    assert (got[up] == DT[t](-9.9)).all(), (what, "the other triangle changed")
    lo = np.tril_indices(n)
    err = float(np.abs(got.astype(WIDE[t]) - want)[lo].max())
    print(f"hermitian function {what}: max err / bound {err / bnd:.4f}")
    assert err <= bnd, (what, err, bnd, err / bnd)
    if t in "cz":
        assert (got.diagonal().imag == 0).all(), (what, "diagonal not exactly real")


@pytest.mark.parametrize("fname", list(FUNCS))
@pytest.mark.parametrize("t,n,nb,bmin", [(t, n, nb, b) for (n, nb, b) in SIZES for t in ("sdcz" if (n, nb) == (150, 64) else "dz")])
def test_function_against_numpy(dlaf, grid, min_band, t, n, nb, bmin, fname):
    f, fmax, lip = FUNCS[fname]
    min_band(bmin)
    a = lower_input(t, n)
    w, sel = dlaf.hermitian_function(grid, "L", a, nb, f)
    want, wref = reference(t, n, f)
    assert sel == (0, n)
    assert np.abs(w - wref).max() <= bound(t, n, 0.0, 1.0), "eigenvalues"
    check_triangle(t, a, want, bound(t, n, fmax, lip), (fname, t, n, nb))


@pytest.mark.parametrize("t", ["d", "z"])
def test_w_is_the_eigensolvers_bit_for_bit(dlaf, grid, t):
    n, nb = 150, 64
    a = lower_input(t, n)
    w, _ = dlaf.hermitian_function(grid, "L", a, nb, lambda x: x)
    b = lower_input(t, n)
    w2 = dlaf.hermitian_eigensolver(grid, "L", b, nb)[0]
    assert np.asarray(w).tobytes() == np.asarray(w2).tobytes()


@pytest.mark.parametrize("t,n,nb", [("s", 150, 64), ("d", 150, 64), ("c", 150, 64), ("z", 150, 64), ("d", 357, 160)])
def test_power_minus_half_orthogonalises(dlaf, grid, t, n, nb):
    """X = A^(-1/2): X A X = I through numpy in the wide type.  X carries the bound of rsqrt (e, say); X A X - I is then
    e A X + X A e to first order, at most 2 n e max|A X| <= 2 n e sqrt(lambda_max) in any element."""
    a = lower_input(t, n)
    w, dropped = dlaf.hermitian_power(grid, "L", a, nb, -0.5)
    assert dropped == 0
    f, fmax, lip = FUNCS["rsqrt"]
    check_triangle(t, a, reference(t, n, f)[0], bound(t, n, fmax, lip), ("power -1/2", t, n))
    x = np.tril(a).astype(WIDE[t])
    x = x + np.tril(x, -1).conj().T
    aw = matrix(t, n)[0].astype(DT[t]).astype(WIDE[t])
    r = x @ aw @ x - np.eye(n)
    assert np.abs(r).max() <= 2 * n * bound(t, n, fmax, lip) * HI ** 0.5, float(np.abs(r).max())


@pytest.mark.parametrize("t", ["d", "z"])
def test_power_with_threshold_drops_and_counts(dlaf, grid, t):
    n, nb = 150, 64
    lam = matrix(t, n)[1]
    j = int(np.searchsorted(lam, 2.0))
    thr = float((lam[j - 1] + lam[j]) / 2)  # midway between two eigenvalues
    a = lower_input(t, n)
    w, dropped = dlaf.hermitian_power(grid, "L", a, nb, -1.0, thr)
    assert dropped == int((lam <= thr).sum()) == j
    f, fmax, lip = FUNCS["inv"]
    want, _ = reference(t, n, lambda x: np.where(x > thr, 1 / np.where(x > thr, x, 1), 0))
    check_triangle(t, a, want, bound(t, n, fmax, lip), ("pinv", t, n))


@pytest.mark.parametrize("by", ["index", "value"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_spectral_projector(dlaf, grid, t, by):
    """f = 1 on the lowest m eigenpairs: trace P = m and P P = P.  P = Z Z^H with Z the computed eigenvectors, so both
    defects are Z (Z^H Z - I) Z^H: the eigensolver's orthogonality error, bounded by n u like its backward error (f' = 0:
    the bound with max |f| = 1 alone); the trace sums n diagonal elements of it."""
    n, nb, m = 150, 64, 37
    lam = matrix(t, n)[1]
    a = lower_input(t, n)
    one = lambda x: np.ones_like(x)  # noqa: E731
    if by == "index":
        w, sel = dlaf.hermitian_function(grid, "L", a, nb, one, eigenvalues_index=(0, m))
    else:
        mu = float((lam[m - 1] + lam[m]) / 2)
        w, sel = dlaf.hermitian_function(grid, "L", a, nb, one, eigenvalues_value=(-np.inf, mu))
    assert sel == (0, m)
    bnd = bound(t, n, 1.0, 0.0)
    assert (a[np.triu_indices(n, 1)] == DT[t](-9.9)).all()
    p = np.tril(a).astype(WIDE[t])
    p = p + np.tril(p, -1).conj().T
    assert abs(float(np.trace(p).real) - m) <= n * bnd, float(np.trace(p).real)
    assert np.abs(p @ p - p).max() <= bnd, float(np.abs(p @ p - p).max() / bnd)
    if t == "z":
        assert (a.diagonal().imag == 0).all()


@pytest.mark.parametrize("t", ["d", "z"])
def test_projector_of_an_inner_range(dlaf, grid, t):
    """eigenvalues_index = (begin, end) with begin inside a tile: the padding columns [b0, begin) take weight 0"""
    n, nb = 150, 64
    a = lower_input(t, n)
    w, sel = dlaf.hermitian_function(grid, "L", a, nb, lambda x: np.ones_like(x), eigenvalues_index=(70, 101))
    assert sel == (70, 101)
    p = np.tril(a).astype(WIDE[t])
    p = p + np.tril(p, -1).conj().T
    bnd = bound(t, n, 1.0, 0.0)
    assert abs(float(np.trace(p).real) - 31) <= n * bnd
    assert np.abs(p @ p - p).max() <= bnd


@pytest.mark.parametrize("t", ["d", "z"])
def test_empty_selection_gives_a_zero_triangle(dlaf, grid, t):
    n, nb = 150, 64
    for kw in ({"eigenvalues_index": (70, 70)}, {"eigenvalues_value": (100.0, 200.0)}):
        a = lower_input(t, n)
        w, sel = dlaf.hermitian_function(grid, "L", a, nb, lambda x: x, **kw)
        assert sel[0] == sel[1]
        assert (a[np.tril_indices(n)] == 0).all() and (a[np.triu_indices(n, 1)] == DT[t](-9.9)).all()
        assert np.abs(w - np.linspace(LO, HI, n)).max() <= bound(t, n, 0.0, 1.0)


@pytest.mark.parametrize("t", ["d", "z"])
def test_resident_chain(dlaf, grid, t):
    """S resident -> hermitian_power_device(-1/2) -> to_general('H') -> two general_multiplication_device calls give
    X S X = I within the bound of test_power_minus_half_orthogonalises, nothing downloaded in between"""
    n, nb = 150, 64
    dt = DT[t]
    s_in = lower_input(t, n)
    S = dlaf.DeviceMatrix(grid, dt, "L", n, nb)
    X = dlaf.DeviceMatrix(grid, dt, "L", n, nb)
    S.upload(s_in)
    X.upload(s_in)
    w, dropped = dlaf.hermitian_power_device(X, -0.5)
    assert dropped == 0
    Sg, Xg, T1, T2 = (dlaf.GeneralDeviceMatrix(grid, dt, n, n, nb) for _ in range(4))
    S.to_general(Sg, "H")
    X.to_general(Xg, "H")
    dlaf.general_multiplication_device("N", "N", 1.0, Xg, Sg, 0.0, T1)
    dlaf.general_multiplication_device("N", "N", 1.0, T1, Xg, 0.0, T2)
    r = np.zeros((n, n), dtype=dt, order="F")
    T2.download(r)
    f, fmax, lip = FUNCS["rsqrt"]
    tol = 2 * n * bound(t, n, fmax, lip) * HI ** 0.5
    assert np.abs(r - np.eye(n)).max() <= tol, float(np.abs(r - np.eye(n)).max() / tol)
    for h in (T2, T1, Xg, Sg, X, S):
        h.close()


def test_function_device_with_selection(dlaf, grid):
    """the resident form of hermitian_function with a value interval equals the host form bit for bit"""
    t, n, nb = "d", 150, 64
    a = lower_input(t, n)
    f = FUNCS["exp"][0]
    w1, sel1 = dlaf.hermitian_function(grid, "L", a, nb, f, eigenvalues_value=(1.0, 5.0))
    b = lower_input(t, n)
    M = dlaf.DeviceMatrix(grid, DT[t], "L", n, nb)
    M.upload(b)
    w2, sel2 = dlaf.hermitian_function_device(M, f, eigenvalues_value=(1.0, 5.0))
    M.download(b)
    assert sel1 == sel2 and w1.tobytes() == w2.tobytes()
    assert a[np.tril_indices(n)].tobytes() == b[np.tril_indices(n)].tobytes()
    M.close()
