"""Hermitian rank-k and rank-2k updates on the GPU (xSYRK / xHERK, xSYR2K / xHER2K) for every type, uplo and trans on
one process, against numpy products in a wider type.

Exact operands: integer-valued entries in [-3, 3] (complex: both parts), alpha = 2, beta = -3 for the rank-k update and
alpha = 2 - 1j (2 for real types) for the rank-2k one.  A product is at most 18 in either part, a sum over k <= 400 of
them at most 7200, the two products of a rank-2k update times alpha plus beta C at most 2 * 7200 * 3 + 9: every
intermediate is an integer below 2^24, exact in all four types in any summation order, so the tests assert equality.
The shapes are the smallest that reach every path of the kernel for blocks of 128 x 128 x 16 (128 x 64, BK 8 for z):
nb = 160, n = 357 gives two blocks per tile dimension with a ragged second one and a ragged last tile, and in z a block
of the diagonal tile that straddles the diagonal; k = 184 a last k tile of 24 (no multiple of BK for s / d / c: the
element kernel), k = 192 the vector kernels; nb = 48 a single ragged block; nb = 33 no 16-byte alignment anywhere.

In every case the other triangle of C is NaN and must come back bit for bit, the diagonal of a complex C carries the
imaginary part 7 on entry and exactly 0 on exit, and the host arrays have a leading dimension larger than the local
rows: the padding of C and all of A and B stay bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = ["s", "d", "c", "z"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
WIDE = {"s": np.float64, "d": np.longdouble, "c": np.complex128, "z": np.clongdouble}
CASES = [(t, tr) for t in TYPES for tr in (("N", "C") if t in "cz" else ("N", "T", "C"))]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def scalars(t, two):
    """(alpha, beta): alpha real for the rank-k update, of the element type for the rank-2k one; beta real"""
    if two:
        return (DT[t](2 - 1j) if t in "cz" else DT[t](2)), -3.0
    return 2.0, -3.0


def integers(rng, t, shape):
    x = rng.integers(-3, 4, shape).astype(np.float64)
    if t in "cz":
        x = x + 1j * rng.integers(-3, 4, shape)
    return np.asfortranarray(x.astype(DT[t]))


def uniform(rng, t, shape):
    x = rng.uniform(-1, 1, shape)
    if t in "cz":
        x = x + 1j * rng.uniform(-1, 1, shape)
    return np.asfortranarray(x.astype(DT[t]))


def operands(make, rng, t, trans, n, k):
    """A, B as stored for trans, and C with the imaginary part 7 on its diagonal"""
    shape = (n, k) if trans == "N" else (k, n)
    c = make(rng, t, (n, n))
    if t in "cz":
        c[np.diag_indices(n)] = c.diagonal().real + 7j
    return make(rng, t, shape), make(rng, t, shape), c


def in_triangle(uplo, n):
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def padded(x, extra, fill):
    store = np.full((x.shape[0] + extra, max(1, x.shape[1])), fill, dtype=x.dtype, order="F")
    view = store[:x.shape[0], :x.shape[1]]
    view[...] = x
    return store, view


def reference(t, two, trans, alpha, a, b, beta, c0):
    """the whole Hermitian result in the wide type (the diagonal of C taken as real)"""
    w = WIDE[t]
    aw, bw = a.astype(w), (b if two else a).astype(w)
    p = aw @ bw.conj().T if trans == "N" else aw.conj().T @ bw
    cw = c0.astype(w)
    if t in "cz":
        cw[np.diag_indices(c0.shape[0])] = cw.diagonal().real
    al = w(alpha)
    r = al * p + (np.conj(al) * p.conj().T if two else 0)
    return r + w(beta) * cw


def run_host(dlaf, grid, t, two, uplo, trans, alpha, a, b, beta, c0, nb):
    """the host entry on padded arrays with the other triangle of C NaN; returns C and asserts that nothing else
    changed and that the diagonal came back real"""
    n = c0.shape[0]
    tri = in_triangle(uplo, n)
    c_in = np.where(tri, c0, np.nan).astype(c0.dtype)
    sa, va = padded(a, 3, np.nan)
    sb, vb = padded(b, 2, np.nan)
    sc, vc = padded(c_in, 5, np.nan)
    before_a, before_b = sa.tobytes(), sb.tobytes()
    pad_c = sc[n:, :].tobytes()
    other = vc[~tri].tobytes()
    if two:
        dlaf.hermitian_rank_2k_update(grid, uplo, trans, alpha, va, vb, beta, vc, nb)
    else:
        dlaf.hermitian_rank_k_update(grid, uplo, trans, alpha, va, beta, vc, nb)
    assert sa.tobytes() == before_a, "A (padding included) changed"
    assert sb.tobytes() == before_b, "B (padding included) changed"
    assert sc[n:, :].tobytes() == pad_c, "the padding rows of C changed"
    assert vc[~tri].tobytes() == other, "the other triangle of C changed"
    return vc.copy(order="F")


def assert_triangle_equal(t, uplo, got, want, what):
    n = got.shape[0]
    tri = in_triangle(uplo, n)
    w = want.astype(DT[t])
    assert np.array_equal(got[tri], w[tri]), (what, int((got[tri] != w[tri]).sum()), np.abs(got[tri] - w[tri]).max())
    if t in "cz":
        assert (got.diagonal().imag == 0).all(), (what, "diagonal not real")


def check_exact(dlaf, grid, t, two, uplo, trans, n, k, nb, seed):
    rng = np.random.default_rng(seed)
    alpha, beta = scalars(t, two)
    a, b, c0 = operands(integers, rng, t, trans, n, k)
    got = run_host(dlaf, grid, t, two, uplo, trans, alpha, a, b, beta, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, two, trans, alpha, a, b, beta, c0), (t, two, uplo, trans, n, k, nb))


@pytest.mark.parametrize("k", [184, 192])
@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t,trans", CASES)
def test_exact_every_type_uplo_trans(dlaf, grid, t, trans, uplo, two, k):
    check_exact(dlaf, grid, t, two, uplo, trans, 357, k, 160, 51)


@pytest.mark.parametrize("nb", [48, 33])
@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_single_block_and_unaligned(dlaf, grid, t, uplo, trans, two, nb):
    check_exact(dlaf, grid, t, two, uplo, trans, 2 * nb + 7, 3 * nb + 8, nb, 52)


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "C"), ("L", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_whole_aligned_tiles(dlaf, grid, t, uplo, trans, two):
    """whole 128-wide blocks only, three k tiles: every block in the vector kernel"""
    check_exact(dlaf, grid, t, two, uplo, trans, 256, 384, 128, 53)


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_exact_k_across_tiles(dlaf, grid, t, trans, two):
    """six k tiles (five whole, one of 8) through the accumulators of one launch"""
    check_exact(dlaf, grid, t, two, "L", trans, 130, 5 * 64 + 8, 64, 54)


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", TYPES)
def test_scalars_and_degenerate_sizes(dlaf, grid, t, uplo, two):
    dt = DT[t]
    rng = np.random.default_rng(55)
    n, k, nb = 150, 90, 64
    alpha, beta = scalars(t, two)
    a, b, c0 = operands(integers, rng, t, "N", n, k)
    nan = np.full_like(c0, np.nan)
    zero = np.zeros_like(c0)
    # beta = 0: a triangle full of NaN is not read
    got = run_host(dlaf, grid, t, two, uplo, "N", alpha, a, b, 0.0, nan, nb)
    assert_triangle_equal(t, uplo, got, reference(t, two, "N", alpha, a, b, 0, zero), "beta = 0 over NaN")
    # alpha = 0: A and B full of NaN are not referenced; the diagonal of beta C comes back real
    an, bn = np.full_like(a, np.nan), np.full_like(b, np.nan)
    got = run_host(dlaf, grid, t, two, uplo, "N", 0 * alpha, an, bn, beta, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, two, "N", 0, zero[:, :1], zero[:, :1], beta, c0), "alpha = 0")
    # k = 0: the triangle becomes beta C; with beta = 0 zero even from NaN
    ak = np.zeros((n, 0), dtype=dt, order="F")
    got = run_host(dlaf, grid, t, two, uplo, "N", alpha, ak, ak, beta, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, two, "N", 0, zero[:, :1], zero[:, :1], beta, c0), "k = 0")
    got = run_host(dlaf, grid, t, two, uplo, "N", alpha, ak, ak, 0.0, nan, nb)
    assert_triangle_equal(t, uplo, got, zero, "k = 0, beta = 0 over NaN")
    # the quick return: alpha = 0 or k = 0 with beta = 1 leaves C bit for bit, the imaginary parts of its diagonal too
    for aa, bb, al in ((an, bn, 0 * alpha), (ak, ak, alpha)):
        got = run_host(dlaf, grid, t, two, uplo, "N", al, aa, bb, 1.0, c0, nb)
        tri = in_triangle(uplo, n)
        assert got[tri].tobytes() == c0[tri].tobytes(), "quick return changed C"
        if t in "cz":
            assert (got.diagonal().imag == 7).all()
    # n = 0 returns
    a0, c00 = np.zeros((0, k), dtype=dt, order="F"), np.zeros((0, 0), dtype=dt, order="F")
    if two:
        dlaf.hermitian_rank_2k_update(grid, uplo, "N", alpha, a0, a0, beta, c00, nb, n=0, k=k)
    else:
        dlaf.hermitian_rank_k_update(grid, uplo, "N", alpha, a0, beta, c00, nb, n=0, k=k)
    # beta = 1, alpha = -1 (the Cholesky's trailing update)
    got = run_host(dlaf, grid, t, two, uplo, "N", -1 + 0 * alpha, a, b, 1.0, c0, nb)
    assert_triangle_equal(t, uplo, got, reference(t, two, "N", -1, a, b, 1, c0), "beta = 1, alpha = -1")


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", TYPES)
def test_upper_and_lower_agree(dlaf, grid, t, trans, two):
    """the two triangles of the same update are conjugate transposes of each other"""
    rng = np.random.default_rng(56)
    n, k, nb = 200, 72, 64
    alpha, beta = scalars(t, two)
    a, b, c0 = operands(integers, rng, t, trans, n, k)
    ch = np.tril(c0) + np.tril(c0, -1).conj().T  # one Hermitian C for both calls
    lo = run_host(dlaf, grid, t, two, "L", trans, alpha, a, b, beta, ch, nb)
    up = run_host(dlaf, grid, t, two, "U", trans, alpha, a, b, beta, ch, nb)
    tri = in_triangle("L", n)
    assert np.array_equal(lo[tri], up.conj().T[tri])


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("t", ["c", "z"])
def test_her2k_alpha_and_its_conjugate_differ(dlaf, grid, t, trans, uplo):
    """alpha and conj(alpha) on the same operands give different results, each its own reference's"""
    n, k, nb = 70, 60, 32
    res = {}
    for alpha in (DT[t](2 - 1j), DT[t](2 + 1j)):
        a, b, c0 = operands(integers, np.random.default_rng(57), t, trans, n, k)
        res[alpha] = run_host(dlaf, grid, t, True, uplo, trans, alpha, a, b, -3.0, c0, nb)
        assert_triangle_equal(t, uplo, res[alpha], reference(t, True, trans, alpha, a, b, -3.0, c0), (alpha, trans, uplo))
    r = list(res.values())
    tri = in_triangle(uplo, n)
    assert not np.array_equal(r[0][tri], r[1][tri])


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("t", TYPES)
def test_uniform_random_operands(dlaf, grid, t, two):
    """Component-wise bound of an inner product in ANY summation order (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., section 3.1), as in test_gpu_general_multiplication.py: fl(sum of m products) differs from the
    sum by at most gamma_m sum |a||b|, gamma_m = m u / (1 - m u), u the unit roundoff of the type.
    Rank-k: m = k terms, then the product with alpha, the product beta c and the final sum add three more roundings to
    the first term and two to the second:  |C - C^| <= (k + 4) u (|alpha| |A| |A|^H + |beta| |C0|)  to first order.
    Rank-2k in one pass (real types, real alpha): both products go into the same accumulators, a sum of m = 2 k terms,
    and the same scalar operations follow:  (2 k + 4) u (|alpha| (|A| |B|^H + |B| |A|^H) + |beta| |C0|).
    Rank-2k in two passes (complex alpha): pass 1 stores fl(alpha acc1 + beta c), pass 2 adds fl(conj(alpha) acc2) to it;
    each accumulator is a sum of k terms only, but what pass 1 stored takes one more rounding in the sum of pass 2: a term
    of the first product sees k + 3 roundings, beta c sees 3 -- both below (2 k + 5) u, the one-pass count plus one.
    A complex product or sum computed from real operations carries a constant below 2 sqrt(2) per operation instead of 1
    (ibid. section 3.6) and the moduli bound the parts: the factor 4.  The reference is computed in the wider type."""
    rng = np.random.default_rng(58)
    n, k, nb = 357, 184, 160
    dt, w = DT[t], WIDE[t]
    alpha = (dt(complex(-1.2, .7)) if t in "cz" else dt(-1.2)) if two else -1.2
    beta = 1.12
    count = (2 * k + (5 if t in "cz" else 4)) if two else k + 4
    real_w = np.longdouble if w in (np.longdouble, np.clongdouble) else np.float64
    for uplo, trans in (("L", "N"), ("U", "C")):
        a, b, c0 = operands(uniform, rng, t, trans, n, k)
        got = run_host(dlaf, grid, t, two, uplo, trans, alpha, a, b, beta, c0, nb)
        want = reference(t, two, trans, alpha, a, b, beta, c0)
        u = float(np.finfo(dt).eps) / 2
        aa, ab = np.abs(a).astype(real_w), np.abs(b if two else a).astype(real_w)
        pm = aa @ ab.T if trans == "N" else aa.T @ ab
        mag = abs(w(alpha)) * (pm + pm.T if two else pm) + abs(beta) * np.abs(c0).astype(real_w)
        bound = (4 if t in "cz" else 1) * count * u * mag
        tri = in_triangle(uplo, n)
        err = np.abs(got.astype(w) - want)
        print(f"uniform {t} {'her2k' if two else 'herk'} {uplo}{trans}: max err / bound {float((err[tri] / bound[tri]).max()):.3f}")
        assert (err[tri] <= bound[tri]).all(), (t, two, uplo, trans, float((err[tri] / bound[tri]).max()))
        if t in "cz":
            assert (got.diagonal().imag == 0).all()


@pytest.mark.parametrize("two", [False, True], ids=["herk", "her2k"])
@pytest.mark.parametrize("trans", ["N", "C"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_resident(dlaf, grid, t, uplo, trans, two):
    """C a DeviceMatrix (uplo U: the conj_view path), A and B GeneralDeviceMatrix: the result equals the host entry's,
    A and B do not change"""
    rng = np.random.default_rng(59)
    n, k, nb = 357, 192, 160
    dt = DT[t]
    alpha, beta = scalars(t, two)
    a, b, c0 = operands(integers, rng, t, trans, n, k)
    host = run_host(dlaf, grid, t, two, uplo, trans, alpha, a, b, beta, c0, nb)
    A = dlaf.GeneralDeviceMatrix(grid, dt, a.shape[0], a.shape[1], nb)
    B = dlaf.GeneralDeviceMatrix(grid, dt, b.shape[0], b.shape[1], nb)
    Cm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    tri = in_triangle(uplo, n)
    c_in = np.asfortranarray(np.where(tri, c0, np.nan).astype(dt))
    A.upload(a)
    B.upload(b)
    Cm.upload(c_in)
    if two:
        dlaf.hermitian_rank_2k_update_device(uplo, trans, alpha, A, B, beta, Cm)
    else:
        dlaf.hermitian_rank_k_update_device(uplo, trans, alpha, A, beta, Cm)
    ms, flops = dlaf.multiplication_profile()
    got = c_in.copy(order="F")
    fa, fb = (np.zeros(x.shape, dtype=dt, order="F") for x in (a, b))
    Cm.download(got)
    A.download(fa)
    B.download(fb)
    assert np.array_equal(got[tri], host[tri]), (t, uplo, trans, two)
    assert got[~tri].tobytes() == c_in[~tri].tobytes()
    assert np.array_equal(fa, a) and np.array_equal(fb, b), "A or B changed"
    assert ms > 0 and flops == (4 if t == "z" else 1) * (2 if two else 1) * k * n * (n + 1), (ms, flops)
    for h in (Cm, B, A):
        h.close()


@pytest.mark.parametrize("t,uplo", [("d", "L"), ("z", "U")])
def test_resident_chain_into_cholesky(dlaf, grid, t, uplo):
    """A -> A^H A + n I -> factorize() without leaving HBM: C = I is uploaded, the update C = 1 A^H A + n C is exact for
    an integer A, and the factor of the same DeviceMatrix is numpy's under the tolerance test_gpu_cholesky.py uses for
    this size (4 (n + 1) err, err = 2 eps for real and 8 eps for complex types; an element passes on its absolute or
    its relative difference)."""
    rng = np.random.default_rng(60)
    n, k, nb = 200, 72, 64
    dt = DT[t]
    a = integers(rng, t, (k, n))
    A = dlaf.GeneralDeviceMatrix(grid, dt, k, n, nb)
    Cm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    A.upload(a)
    Cm.upload(np.asfortranarray(np.eye(n, dtype=dt)))
    dlaf.hermitian_rank_k_update_device(uplo, "C", 1.0, A, float(n), Cm)
    full = a.conj().T @ a + n * np.eye(n, dtype=dt)  # exact: integers below 2^24
    got = np.zeros((n, n), dtype=dt, order="F")
    Cm.download(got)
    tri = in_triangle(uplo, n)
    assert np.array_equal(got[tri], full[tri])
    assert Cm.factorize() == 0
    Cm.download(got)
    low = np.linalg.cholesky(full)
    want = low if uplo == "L" else low.conj().T
    tol = 4 * (n + 1) * (8 if t == "z" else 2) * float(np.finfo(dt).eps)
    diff = np.abs(got - want)[tri]
    big = np.maximum(np.abs(got), np.abs(want))[tri]
    assert ((diff < tol) | (diff < tol * big)).all(), float(diff.max())
    for h in (Cm, A):
        h.close()


@pytest.mark.parametrize("t", TYPES)
def test_pxherk_and_pxher2k(dlaf, grid, t):
    """p?syrk / p?herk and p?syr2k / p?her2k with 9-int descriptors on a 1 x 1 grid"""
    rng = np.random.default_rng(61)
    n, k, nb = 150, 90, 32
    for two, (uplo, trans) in ((False, ("L", "N")), (True, ("U", "C"))):
        alpha, beta = scalars(t, two)
        a, b, c0 = operands(integers, rng, t, trans, n, k)
        tri = in_triangle(uplo, n)
        c = np.asfortranarray(np.where(tri, c0, np.nan).astype(DT[t]))
        other = c[~tri].tobytes()
        desca = [1, grid.context, a.shape[0], a.shape[1], nb, nb, 0, 0, a.shape[0]]
        descc = [1, grid.context, n, n, nb, nb, 0, 0, n]
        if two:
            dlaf.pxher2k(uplo, trans, n, k, alpha, a, 1, 1, desca, b, 1, 1, desca, beta, c, 1, 1, descc)
        else:
            dlaf.pxherk(uplo, trans, n, k, alpha, a, 1, 1, desca, beta, c, 1, 1, descc)
        assert_triangle_equal(t, uplo, c, reference(t, two, trans, alpha, a, b, beta, c0), (t, two))
        assert c[~tri].tobytes() == other


@pytest.mark.parametrize("setup,call,needle", [
    ("A = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'U', 6, 2)",
     "d.hermitian_rank_k_update_device('L', 'N', 1.0, A, 0.0, Cm)",
     "hermitian rank-k update: uplo 'L' but the resident matrix holds its 'U' triangle"),
    ("A = d.GeneralDeviceMatrix(g, np.float32, 6, 4, 2); Cm = d.DeviceMatrix(g, np.float64, 'L', 6, 2)",
     "d.hermitian_rank_k_update_device('L', 'N', 1.0, A, 0.0, Cm)",
     "hermitian rank-k update: operands of different element types (A 's', C 'd')"),
    ("g2 = d.Grid.single(); A = d.GeneralDeviceMatrix(g2, np.float64, 6, 4, 2); B = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2); "
     "Cm = d.DeviceMatrix(g, np.float64, 'L', 6, 2)",
     "d.hermitian_rank_2k_update_device('L', 'N', 1.0, A, B, 0.0, Cm)",
     "hermitian rank-2k update: the operands live on different contexts"),
    ("A = d.GeneralDeviceMatrix(g, np.complex128, 4, 6, 2); Cm = d.DeviceMatrix(g, np.complex128, 'L', 6, 2)",
     "d.hermitian_rank_k_update_device('L', 'T', 1.0, A, 0.0, Cm)",
     "hermitian rank-k update: trans 'T' on a complex type"),
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
