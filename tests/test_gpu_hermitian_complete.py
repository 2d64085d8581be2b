"""hermitian_complete and the resident conversions between a DeviceMatrix (one triangle) and a general resident matrix
on the GPU, one process: both uplo, both kinds, all four types, in place through the host entry (padded arrays) and
the resident one.  A completion moves bits (kind H flips the sign of the imaginary part), so every comparison is an
equality.  The shapes (nb, n) are those of tests/test_gpu_general_addition.py made square -- sub-blocks of 64 (32 for z):
(160, 357) several sub-blocks with a ragged one and diagonal sub-blocks in ragged tiles, (48, 100) and (24, 50) a single
ragged sub-block, (33, 70) and (50, 110) the element path, (64, 64) one tile, (32, 1) one element.

On entry the other triangle is NaN; the source triangle (and, for kind S, the diagonal) must come back bit for bit; for
kind H every second diagonal element carries a NaN imaginary part on entry and exactly 0 on exit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = ["s", "d", "c", "z"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
SHAPES = [(160, 357), (48, 100), (24, 50), (33, 70), (50, 110), (64, 64), (32, 1)]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def fortran(x, dtype=None):
    out = np.empty(x.shape, dtype=dtype or x.dtype, order="F")
    out[...] = x
    return out


def uniform(rng, t, shape):
    x = rng.uniform(-1, 1, shape)
    if t in "cz":
        x = x + 1j * rng.uniform(-1, 1, shape)
    return fortran(x, DT[t])


def integers(rng, t, shape):
    x = rng.integers(-3, 4, shape).astype(np.float64)
    if t in "cz":
        x = x + 1j * rng.integers(-3, 4, shape)
    return fortran(x, DT[t])


def triangle(uplo, n, strict=False):
    i, j = np.indices((n, n))
    if strict:
        return i > j if uplo == "L" else i < j
    return i >= j if uplo == "L" else i <= j


def completed(t, uplo, kind, a):
    """the full matrix whose uplo triangle a holds; kind H: conjugated mirror and a real diagonal, S: plain mirror, T:
    zeros in the other triangle"""
    n = a.shape[0]
    tri = np.where(triangle(uplo, n), a, 0)
    strict = np.where(triangle(uplo, n, True), a, 0)
    if kind == "T":
        return fortran(tri, DT[t])
    full = tri + (strict.conj().T if kind == "H" else strict.T)
    if kind == "H" and t in "cz":
        full[np.diag_indices(n)] = full.diagonal().real
    return fortran(full, DT[t])


def source(rng, t, uplo, kind, n):
    a = uniform(rng, t, (n, n))
    if kind == "H" and t in "cz":
        odd = np.arange(1, n, 2)
        a.imag[odd, odd] = np.nan
    return fortran(np.where(triangle(uplo, n), a, np.nan), DT[t])


def padded(x, extra, fill):
    store = np.full((x.shape[0] + extra, max(1, x.shape[1])), fill, dtype=x.dtype, order="F")
    view = store[:x.shape[0], :x.shape[1]]
    view[...] = x
    return store, view


def check(t, uplo, kind, a_in, got, how):
    n = a_in.shape[0]
    kept = triangle(uplo, n, strict=(kind == "H" and t in "cz"))
    assert got[kept].tobytes() == a_in[kept].tobytes(), f"{how}: the source triangle changed"
    want = completed(t, uplo, kind, np.where(np.isnan(a_in.imag) if t in "cz" else False, a_in.real, a_in))
    assert np.array_equal(got, want), (how, np.argwhere(got != want)[:5])
    if kind == "H" and t in "cz":
        assert got.diagonal().imag.tobytes() == np.zeros(n, got.real.dtype).tobytes(), f"{how}: diagonal not real"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("kind", ["H", "S"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("nb,n", SHAPES)
def test_complete_in_place(dlaf, grid, nb, n, uplo, kind, t):
    rng = np.random.default_rng(nb + n)
    a_in = source(rng, t, uplo, kind, n)
    store, view = padded(a_in, 4, np.nan)
    pad = store[n:, :].tobytes()
    dlaf.hermitian_complete(grid, uplo, kind, view, nb, n=n)
    assert store[n:, :].tobytes() == pad, "the padding rows changed"
    check(t, uplo, kind, a_in, fortran(view), "host")
    g = dlaf.GeneralDeviceMatrix(grid, DT[t], n, n, nb)
    g.upload(a_in)
    dlaf.hermitian_complete_device(uplo, kind, g)
    out = fortran(np.zeros_like(a_in))
    g.download(out)
    g.close()
    check(t, uplo, kind, a_in, out, "resident")


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("nb,n", [(160, 357), (33, 70), (24, 50)])
def test_conversions(dlaf, grid, nb, n, uplo, t):
    rng = np.random.default_rng(2 * nb + n)
    a = uniform(rng, t, (n, n))
    tri = triangle(uplo, n)
    a_in = fortran(np.where(tri, a, np.nan), DT[t])
    D = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    G = dlaf.GeneralDeviceMatrix(grid, DT[t], n, n, nb)
    D.upload(a_in)
    for kind in ("H", "S", "T"):
        G.upload(fortran(np.full((n, n), np.nan), DT[t]))
        D.to_general(G, kind)
        out = fortran(np.zeros((n, n)), DT[t])
        G.download(out)
        want = completed(t, uplo, kind, a_in)
        assert np.array_equal(out, want), (kind, np.argwhere(out != want)[:5])
        if kind == "T":
            assert out[~tri].tobytes() == np.zeros((n, n), DT[t])[~tri].tobytes(), "not exact zeros"
    # the other way: the triangle of a general matrix into the DeviceMatrix, shown by its download
    b = uniform(rng, t, (n, n))
    G.upload(b)
    D.from_general(G)
    got = fortran(np.full((n, n), np.nan), DT[t])
    D.download(got)
    assert got[tri].tobytes() == b[tri].tobytes()
    assert np.isnan(got[~tri]).all(), "download wrote outside the triangle"
    back = fortran(np.zeros((n, n)), DT[t])
    G.download(back)
    assert back.tobytes() == b.tobytes(), "the general matrix changed"
    D.close()
    G.close()


@pytest.mark.parametrize("t,uplo", [("d", "L"), ("z", "U"), ("d", "U"), ("z", "L")])
def test_chain_rank_update_to_general_to_multiplication(dlaf, grid, t, uplo):
    """hermitian_rank_k_update_device -> to_general('H') -> general_multiplication_device without leaving HBM, against
    numpy; integer operands keep every intermediate an integer below 2^53: equality"""
    rng = np.random.default_rng(8)
    n, k, nb = 357, 16, 160
    a, x = integers(rng, t, (n, k)), integers(rng, t, (n, 40))
    A = dlaf.GeneralDeviceMatrix(grid, DT[t], n, k, nb)
    X = dlaf.GeneralDeviceMatrix(grid, DT[t], n, 40, nb)
    P = dlaf.GeneralDeviceMatrix(grid, DT[t], n, 40, nb)
    G = dlaf.GeneralDeviceMatrix(grid, DT[t], n, n, nb)
    C = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    A.upload(a)
    X.upload(x)
    dlaf.hermitian_rank_k_update_device(uplo, "N", 1.0, A, 0.0, C)
    C.to_general(G, "H")
    dlaf.general_multiplication_device("N", "N", 1.0, G, X, 0.0, P)
    got = fortran(np.zeros((n, 40)), DT[t])
    P.download(got)
    assert np.array_equal(got, (a @ a.conj().T) @ x)
    for h in (A, X, P, G, C):
        h.close()


@pytest.mark.parametrize("t,uplo", [("d", "L"), ("z", "U")])
def test_chain_multiplication_from_general_to_cholesky(dlaf, grid, t, uplo):
    """general_multiplication_device (A^H A + n I) -> from_general -> factorize() without leaving HBM.  The product is
    exact for an integer A; the factor is the host route's (download, cholesky_factorization on the host array) and
    numpy's under the tolerance test_gpu_cholesky.py uses for this size (4 (n + 1) err, err = 2 eps real / 8 eps
    complex; an element passes on its absolute or its relative difference)."""
    rng = np.random.default_rng(9)
    n, nb = 357, 160
    dt = DT[t]
    a = integers(rng, t, (n, n))
    A = dlaf.GeneralDeviceMatrix(grid, dt, n, n, nb)
    G = dlaf.GeneralDeviceMatrix(grid, dt, n, n, nb)
    D = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    A.upload(a)
    G.upload(fortran(np.eye(n), dt))
    dlaf.general_multiplication_device("C", "N", 1.0, A, A, float(n), G)
    full = a.conj().T @ a + n * np.eye(n, dtype=dt)
    host = fortran(np.zeros((n, n)), dt)
    G.download(host)
    assert np.array_equal(host, full)
    D.from_general(G)
    assert D.factorize() == 0
    got = fortran(np.zeros((n, n)), dt)
    D.download(got)
    dlaf.cholesky_factorization(grid, uplo, host, nb)
    low = np.linalg.cholesky(full)
    tri = triangle(uplo, n)
    tol = 4 * (n + 1) * (8 if t == "z" else 2) * float(np.finfo(dt).eps)
    for want in (host, low if uplo == "L" else low.conj().T):
        diff = np.abs(got - want)[tri]
        big = np.maximum(np.abs(got), np.abs(want))[tri]
        assert ((diff < tol) | (diff < tol * big)).all(), float(diff.max())
    for h in (A, G, D):
        h.close()
