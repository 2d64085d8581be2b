"""The weighted Hermitian rank-k update C = alpha A D A^H + beta C (trans N) / alpha A^H D A + beta C (trans C), D a real
diagonal of any sign, on the GPU for every type, uplo and trans on one process, against numpy products in a wider type.
Modelled on test_gpu_hermitian_rank_update.py, whose shapes (the smallest that reach every path of a 128 x 128 x 16 block;
128 x 64 with BK 8 for z) and helpers it reuses.

Exact operands: A and C0 are integers in [-3, 3] (complex: both parts), d integers in [-3, 3] from the generator, so zeros
and negative weights occur; alpha = 2, beta = -3.  A weighted product is at most 2 * 3 * 3 * 3 = 54 in either part, a sum
over k <= 400 of them at most 21600, times alpha plus beta C below 2^24: exact in all four types in any summation order,
so the tests assert equality.

In every case the other triangle of C is NaN and must come back bit for bit, the diagonal of a complex C carries the
imaginary part 7 on entry and exactly 0 on exit, and the host arrays have padded leading dimensions: the padding of C,
all of A and d stay bit for bit."""
import numpy as np
import pytest

from test_gpu_hermitian_rank_update import (CASES, DT, TYPES, WIDE, in_triangle, integers, operands, padded, uniform)

pytestmark = pytest.mark.gpu

ALPHA, BETA = 2.0, -3.0


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def weights(rng, t, k):
    return rng.integers(-3, 4, k).astype(DT[t](0).real.dtype)


def reference(t, trans, alpha, a, d, beta, c0):
    """the whole Hermitian result in the wide type (the diagonal of C taken as real)"""
    w = WIDE[t]
    aw = a.astype(w)
    dw = np.asarray(d).astype(w)
    p = (aw * dw[None, :]) @ aw.conj().T if trans == "N" else (aw.conj().T * dw[None, :]) @ aw
    cw = c0.astype(w)
    if t in "cz":
        cw[np.diag_indices(c0.shape[0])] = cw.diagonal().real
    return w(alpha) * p + w(beta) * cw


def run_host(dlaf, grid, t, uplo, trans, alpha, a, d, beta, c0, nb):
    """the host entry on padded arrays with the other triangle of C NaN; returns C and asserts that nothing else changed"""
    n = c0.shape[0]
    tri = in_triangle(uplo, n)
    c_in = np.where(tri, c0, np.nan).astype(c0.dtype)
    sa, va = padded(a, 3, np.nan)
    sc, vc = padded(c_in, 5, np.nan)
    dd = np.array(d, copy=True)
    before_a, before_d = sa.tobytes(), dd.tobytes()
    pad_c = sc[n:, :].tobytes()
    other = vc[~tri].tobytes()
    dlaf.hermitian_weighted_rank_k_update(grid, uplo, trans, alpha, va, dd, beta, vc, nb)
    assert sa.tobytes() == before_a, "A (padding included) changed"
    assert dd.tobytes() == before_d, "d changed"
    assert sc[n:, :].tobytes() == pad_c, "the padding rows of C changed"
    assert vc[~tri].tobytes() == other, "the other triangle of C changed"
    return vc.copy(order="F")


def assert_triangle_equal(t, uplo, got, want, what):
    tri = in_triangle(uplo, got.shape[0])
    w = want.astype(DT[t])
    assert np.array_equal(got[tri], w[tri]), (what, int((got[tri] != w[tri]).sum()), np.abs(got[tri] - w[tri]).max())
    if t in "cz":
        assert (got.diagonal().imag == 0).all(), (what, "diagonal not real")


def check_exact(dlaf, grid, t, uplo, trans, n, k, nb, seed):
    rng = np.random.default_rng(seed)
    a, _, c0 = operands(integers, rng, t, trans, n, k)
    d = weights(rng, t, k)
    got = run_host(dlaf, grid, t, uplo, trans, ALPHA, a, d, BETA, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, trans, ALPHA, a, d, BETA, c0), (t, uplo, trans, n, k, nb))


@pytest.mark.parametrize("k", [184, 192])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t,trans", CASES)
def test_exact_every_type_uplo_trans(dlaf, grid, t, trans, uplo, k):
    """k = 184: a last k tile of 24 (the element kernel for s / d / c); k = 192: the vector kernels"""
    check_exact(dlaf, grid, t, uplo, trans, 357, k, 160, 71)


@pytest.mark.parametrize("nb", [48, 33])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_single_block_and_unaligned(dlaf, grid, t, uplo, trans, nb):
    check_exact(dlaf, grid, t, uplo, trans, 2 * nb + 7, 3 * nb + 8, nb, 72)


@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C"), ("L", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_whole_aligned_tiles(dlaf, grid, t, uplo, trans):
    """whole 128-wide blocks only, three k tiles: every block in the vector kernel"""
    check_exact(dlaf, grid, t, uplo, trans, 256, 384, 128, 73)


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_exact_k_across_tiles(dlaf, grid, t, trans):
    """six k tiles (five whole, one of 8): the weight pointer across tiles and the ragged last one"""
    check_exact(dlaf, grid, t, "L", trans, 130, 5 * 64 + 8, 64, 74)


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_one_hot_weights(dlaf, grid, t, trans):
    """d = e_j: the result is alpha a_j a_j^H exactly -- pins WHICH k a weight hits: the first and last k of a slab (BK 16
    for d, 8 for z), of a k tile, of the update"""
    rng = np.random.default_rng(75)
    n, k, nb = 130, 328, 64
    bk = 8 if t == "z" else 16
    a, _, c0 = operands(integers, rng, t, trans, n, k)
    for j in (0, bk - 1, bk, nb - 1, nb, k - 1):
        d = np.zeros(k, dtype=DT[t](0).real.dtype)
        d[j] = 1
        got = run_host(dlaf, grid, t, "L", trans, ALPHA, a, d, 0.0, c0, nb)
        col = (a[:, j] if trans == "N" else a[j, :].conj()).astype(WIDE[t])
        assert_triangle_equal(t, "L", got, ALPHA * np.outer(col, col.conj()), (t, trans, j))


@pytest.mark.parametrize("k", [184, 192])
@pytest.mark.parametrize("t,trans", CASES)
def test_unit_weights_are_the_rank_k_update_bit_for_bit(dlaf, grid, t, trans, k):
    """d = ones on uniform random operands: the triangle is bit-identical to hermitian_rank_k_update's on the same
    inputs (a multiplication by 1 is exact, and nothing else differs)"""
    rng = np.random.default_rng(76)
    n, nb = 357, 160
    a, _, c0 = operands(uniform, rng, t, trans, n, k)
    d = np.ones(k, dtype=DT[t](0).real.dtype)
    for uplo in ("L", "U"):
        tri = in_triangle(uplo, n)
        got = run_host(dlaf, grid, t, uplo, trans, -1.2, a, d, 1.12, c0, nb)
        plain = np.asfortranarray(np.where(tri, c0, np.nan).astype(c0.dtype))
        dlaf.hermitian_rank_k_update(grid, uplo, trans, -1.2, a, 1.12, plain, nb)
        assert got[tri].tobytes() == plain[tri].tobytes(), (t, trans, uplo, k)


@pytest.mark.parametrize("t", TYPES)
def test_uniform_random_operands(dlaf, grid, t):
    """The component-wise bound of test_gpu_hermitian_rank_update.py (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., section 3.1: any summation order) with ONE more rounding per term, the multiplication by the
    weight:  |C - C^| <= (k + 5) u (|alpha| |A| |D| |A|^H + |beta| |C0|), x 4 for complex types."""
    rng = np.random.default_rng(77)
    n, k, nb = 357, 184, 160
    dt, w = DT[t], WIDE[t]
    alpha, beta = -1.2, 1.12
    real_w = np.longdouble if w in (np.longdouble, np.clongdouble) else np.float64
    for uplo, trans in (("L", "N"), ("U", "C")):
        a, _, c0 = operands(uniform, rng, t, trans, n, k)
        d = rng.uniform(-2, 2, k).astype(dt(0).real.dtype)
        got = run_host(dlaf, grid, t, uplo, trans, alpha, a, d, beta, c0, nb)
        want = reference(t, trans, alpha, a, d, beta, c0)
        u = float(np.finfo(dt).eps) / 2
        aa, ad = np.abs(a).astype(real_w), np.abs(d).astype(real_w)
        pm = (aa * ad[None, :]) @ aa.T if trans == "N" else (aa.T * ad[None, :]) @ aa
        bound = (4 if t in "cz" else 1) * (k + 5) * u * (abs(alpha) * pm + abs(beta) * np.abs(c0).astype(real_w))
        tri = in_triangle(uplo, n)
        err = np.abs(got.astype(w) - want)
        print(f"uniform {t} weighted {uplo}{trans}: max err / bound {float((err[tri] / bound[tri]).max()):.3f}")
        assert (err[tri] <= bound[tri]).all(), (t, uplo, trans, float((err[tri] / bound[tri]).max()))
        if t in "cz":
            assert (got.diagonal().imag == 0).all()


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", TYPES)
def test_scalars_and_degenerate_sizes(dlaf, grid, t, uplo):
    dt = DT[t]
    rdt = dt(0).real.dtype
    rng = np.random.default_rng(78)
    n, k, nb = 150, 90, 64
    a, _, c0 = operands(integers, rng, t, "N", n, k)
    d = weights(rng, t, k)
    nan, zero = np.full_like(c0, np.nan), np.zeros_like(c0)
    tri = in_triangle(uplo, n)
    # beta = 0: a triangle full of NaN is not read
    got = run_host(dlaf, grid, t, uplo, "N", ALPHA, a, d, 0.0, nan, nb)
    assert_triangle_equal(t, uplo, got, reference(t, "N", ALPHA, a, d, 0, zero), "beta = 0 over NaN")
    # alpha = 0: A and d full of NaN are not referenced; the diagonal of beta C comes back real
    an, dn = np.full_like(a, np.nan), np.full(k, np.nan, dtype=rdt)
    got = run_host(dlaf, grid, t, uplo, "N", 0.0, an, dn, BETA, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, "N", 0, zero[:, :1], [0], BETA, c0), "alpha = 0")
    # k = 0: the triangle becomes beta C; with beta = 0 zero even from NaN
    ak, dk = np.zeros((n, 0), dtype=dt, order="F"), np.zeros(0, dtype=rdt)
    got = run_host(dlaf, grid, t, uplo, "N", ALPHA, ak, dk, BETA, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, "N", 0, zero[:, :1], [0], BETA, c0), "k = 0")
    got = run_host(dlaf, grid, t, uplo, "N", ALPHA, ak, dk, 0.0, nan, nb)
    assert_triangle_equal(t, uplo, got, zero, "k = 0, beta = 0 over NaN")
    # the quick return: alpha = 0 or k = 0 with beta = 1 leaves C bit for bit, the imaginary parts of its diagonal too
    for aa, dd, al in ((an, dn, 0.0), (ak, dk, ALPHA)):
        got = run_host(dlaf, grid, t, uplo, "N", al, aa, dd, 1.0, c0, nb)
        assert got[tri].tobytes() == c0[tri].tobytes(), "quick return changed C"
        if t in "cz":
            assert (got.diagonal().imag == 7).all()
    # n = 0 returns
    a0, c00 = np.zeros((0, k), dtype=dt, order="F"), np.zeros((0, 0), dtype=dt, order="F")
    dlaf.hermitian_weighted_rank_k_update(grid, uplo, "N", ALPHA, a0, d, BETA, c00, nb, n=0, k=k)
    # a zero weight does NOT unreference its column: 0 * NaN is NaN, as documented -- every element of the triangle whose
    # row AND column of A meet the NaN column
    ax, dx = a.copy(order="F"), d.copy()
    ax[:, 5] = np.nan
    dx[5] = 0
    got = run_host(dlaf, grid, t, uplo, "N", ALPHA, ax, dx, BETA, c0, nb)
    assert np.isnan(got[tri]).all(), "a zero weight hid a NaN column"


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", TYPES)
def test_upper_and_lower_agree(dlaf, grid, t, trans):
    """the two triangles of the same update are conjugate transposes of each other"""
    rng = np.random.default_rng(79)
    n, k, nb = 200, 72, 64
    a, _, c0 = operands(integers, rng, t, trans, n, k)
    d = weights(rng, t, k)
    ch = np.tril(c0) + np.tril(c0, -1).conj().T
    lo = run_host(dlaf, grid, t, "L", trans, ALPHA, a, d, BETA, ch, nb)
    up = run_host(dlaf, grid, t, "U", trans, ALPHA, a, d, BETA, ch, nb)
    tri = in_triangle("L", n)
    assert np.array_equal(lo[tri], up.conj().T[tri])


@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_resident(dlaf, grid, t, uplo, trans):
    """C a DeviceMatrix (uplo U: the conj_view path), A a GeneralDeviceMatrix: the result equals the host entry's, A does
    not change, the profile hook reports herk's flops"""
    rng = np.random.default_rng(80)
    n, k, nb = 357, 192, 160
    dt = DT[t]
    a, _, c0 = operands(integers, rng, t, trans, n, k)
    d = weights(rng, t, k)
    host = run_host(dlaf, grid, t, uplo, trans, ALPHA, a, d, BETA, c0, nb)
    A = dlaf.GeneralDeviceMatrix(grid, dt, a.shape[0], a.shape[1], nb)
    Cm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    tri = in_triangle(uplo, n)
    c_in = np.asfortranarray(np.where(tri, c0, np.nan).astype(dt))
    A.upload(a)
    Cm.upload(c_in)
    dlaf.hermitian_weighted_rank_k_update_device(uplo, trans, ALPHA, A, d, BETA, Cm)
    ms, flops = dlaf.multiplication_profile()
    got = c_in.copy(order="F")
    fa = np.zeros(a.shape, dtype=dt, order="F")
    Cm.download(got)
    A.download(fa)
    assert np.array_equal(got[tri], host[tri]), (t, uplo, trans)
    assert got[~tri].tobytes() == c_in[~tri].tobytes()
    assert np.array_equal(fa, a), "A changed"
    assert ms > 0 and flops == (4 if t == "z" else 1) * k * n * (n + 1), (ms, flops)
    for h in (Cm, A):
        h.close()


@pytest.mark.parametrize("setup,call,needle", [
    ("A = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'U', 6, 2)",
     "d.hermitian_weighted_rank_k_update_device('L', 'N', 1.0, A, np.ones(4), 0.0, Cm)",
     "hermitian weighted rank-k update: uplo 'L' but the resident matrix holds its 'U' triangle"),
    ("A = d.GeneralDeviceMatrix(g, np.float32, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'L', 6, 2)",
     "d.hermitian_weighted_rank_k_update_device('L', 'N', 1.0, A, np.ones(4), 0.0, Cm)",
     "hermitian weighted rank-k update: operands of different element types (A 's', C 'd')"),
    ("g2 = d.Grid.single(); A = d.GeneralDeviceMatrix(g2, np.float64, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'L', 6, 2)",
     "d.hermitian_weighted_rank_k_update_device('L', 'N', 1.0, A, np.ones(4), 0.0, Cm)",
     "hermitian weighted rank-k update: the operands live on different contexts"),
    ("A = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'L', 6, 2)",
     "d.hermitian_weighted_rank_k_update_device('L', 'N', 1.0, A, None, 0.0, Cm)",
     "hermitian weighted rank-k update: the weights d are null (k = 4, alpha != 0)"),
])
def test_resident_refusals(setup, call, needle):
    """the refusals that need a resident matrix terminate the process with the routine's message (one process each)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import numpy as np, dla_future_amd as d\nd.initialize()\ng = d.Grid.single()\n" + setup.replace("; ", "\n") + "\n" +
            call + "\nprint('survived')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    assert needle in r.stderr, r.stderr[-800:]
