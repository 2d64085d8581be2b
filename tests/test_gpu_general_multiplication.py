"""General multiplication on the GPU: C = beta C + alpha op(A) op(B) for every op pair and type on one process, against
numpy products in a wider type.

Exact operands: integer-valued entries in [-3, 3] (complex: both parts) and small integer alpha, beta.  A product is at
most 18 in either part, a sum over k <= 400 of them at most 7200, times alpha and plus beta C below 2^16: every
intermediate is an integer below 2^24, exact in all four types in any summation order, so the tests assert equality.
The shapes are the smallest that reach every loader of the kernel for blocks of 128 x 128 x 16 (64 wide, BK 8 for z):
nb = 160, m = 357, n = 165 gives two blocks per tile with a ragged second one and ragged last tiles on m and n; k = 184
a last k tile of 24 (no multiple of BK for s / d / c -- the element kernel everywhere -- a multiple for z: the vector
kernel on the whole interior blocks), k = 192 a last k tile of 32 (the vector kernels of every type); nb = 48 a single
ragged block; nb = 33 no 16-byte alignment anywhere.

Host arrays have a leading dimension larger than the local rows: the padding of C and all of A and B stay bit for bit."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = ["s", "d", "c", "z"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
WIDE = {"s": np.float64, "d": np.longdouble, "c": np.complex128, "z": np.clongdouble}
OPS = ["N", "T", "C"]
PAIRS = list(itertools.product(OPS, OPS))
SHAPE = (357, 165, 184)


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def scalars(t):
    dt = DT[t]
    return (dt(2 - 1j), dt(-1 + 2j)) if t in "cz" else (dt(2), dt(-3))


def op_of(x, o):
    return x if o == "N" else x.T if o == "T" else x.conj().T


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


def operands(make, rng, t, opa, opb, m, n, k):
    """A, B as stored for the ops, and C"""
    return (make(rng, t, (m, k) if opa == "N" else (k, m)), make(rng, t, (k, n) if opb == "N" else (n, k)),
            make(rng, t, (m, n)))


def padded(x, extra, fill):
    """x inside a store with `extra` more rows, the padding filled with `fill`; (store, view)"""
    store = np.full((x.shape[0] + extra, max(1, x.shape[1])), fill, dtype=x.dtype, order="F")
    view = store[:x.shape[0], :x.shape[1]]
    view[...] = x
    return store, view


def reference(t, opa, opb, alpha, a, b, beta, c0):
    w = WIDE[t]
    return w(beta) * c0.astype(w) + w(alpha) * (op_of(a.astype(w), opa) @ op_of(b.astype(w), opb))


def run_host(dlaf, grid, t, opa, opb, alpha, a, b, beta, c0, nb):
    """the host entry on padded arrays; returns C and asserts that nothing else changed"""
    sa, va = padded(a, 3, np.nan)
    sb, vb = padded(b, 2, np.nan)
    sc, vc = padded(c0, 5, np.nan)
    before_a, before_b = sa.tobytes(), sb.tobytes()
    pad_c = sc[c0.shape[0]:, :].tobytes()
    dlaf.general_multiplication(grid, opa, opb, alpha, va, vb, beta, vc, nb)
    assert sa.tobytes() == before_a, "A (padding included) changed"
    assert sb.tobytes() == before_b, "B (padding included) changed"
    assert sc[c0.shape[0]:, :].tobytes() == pad_c, "the padding rows of C changed"
    return vc.copy(order="F")


def check_exact(dlaf, grid, t, opa, opb, m, n, k, nb, seed):
    rng = np.random.default_rng(seed)
    alpha, beta = scalars(t)
    a, b, c0 = operands(integers, rng, t, opa, opb, m, n, k)
    got = run_host(dlaf, grid, t, opa, opb, alpha, a, b, beta, c0, nb)
    want = reference(t, opa, opb, alpha, a, b, beta, c0).astype(DT[t])
    assert np.array_equal(got, want), (t, opa, opb, m, n, k, nb, int((got != want).sum()), np.abs(got - want).max())


@pytest.mark.parametrize("k", [184, 192])
@pytest.mark.parametrize("opa,opb", PAIRS)
@pytest.mark.parametrize("t", TYPES)
def test_exact_every_op_pair(dlaf, grid, t, opa, opb, k):
    check_exact(dlaf, grid, t, opa, opb, SHAPE[0], SHAPE[1], k, 160, 31)


@pytest.mark.parametrize("nb", [48, 33])
@pytest.mark.parametrize("opa,opb", [("N", "N"), ("C", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_single_block_and_unaligned(dlaf, grid, t, opa, opb, nb):
    check_exact(dlaf, grid, t, opa, opb, 2 * nb + 7, nb + 5, 3 * nb + 8, nb, 32)


@pytest.mark.parametrize("opa", ["N", "T"])
@pytest.mark.parametrize("t", ["d", "z"])
def test_exact_k_across_tiles(dlaf, grid, t, opa):
    """six k tiles (five whole, one of 8) through the accumulators of one launch"""
    check_exact(dlaf, grid, t, opa, "N", 130, 70, 5 * 64 + 8, 64, 33)


@pytest.mark.parametrize("opa,opb", [("N", "N"), ("T", "C")])
@pytest.mark.parametrize("t", TYPES)
def test_exact_whole_aligned_tiles(dlaf, grid, t, opa, opb):
    """whole 128-wide blocks only, three k tiles: every block in the vector kernel"""
    check_exact(dlaf, grid, t, opa, opb, 256, 128, 384, 128, 34)


@pytest.mark.parametrize("t", TYPES)
def test_scalars_and_degenerate_sizes(dlaf, grid, t):
    dt = DT[t]
    rng = np.random.default_rng(35)
    m, n, k, nb = 150, 70, 90, 64
    alpha, beta = scalars(t)
    a, b, c0 = operands(integers, rng, t, "N", "N", m, n, k)
    nan = np.full_like(c0, np.nan)
    # beta = 0: a C full of NaN is not read
    got = run_host(dlaf, grid, t, "N", "N", alpha, a, b, dt(0), nan, nb)
    assert np.array_equal(got, reference(t, "N", "N", alpha, a, b, 0, np.zeros_like(c0)).astype(dt)), "beta = 0 over NaN"
    # alpha = 0: A and B full of NaN are not referenced
    got = run_host(dlaf, grid, t, "N", "N", dt(0), np.full_like(a, np.nan), np.full_like(b, np.nan), beta, c0, nb)
    assert np.array_equal(got, (WIDE[t](beta) * c0.astype(WIDE[t])).astype(dt)), "alpha = 0 with NaN operands"
    # k = 0: C = beta C; with beta = 0 a zero C even from NaN
    ak, bk = np.zeros((m, 0), dtype=dt, order="F"), np.zeros((0, n), dtype=dt, order="F")
    got = run_host(dlaf, grid, t, "N", "N", alpha, ak, bk, beta, c0, nb)
    assert np.array_equal(got, (WIDE[t](beta) * c0.astype(WIDE[t])).astype(dt)), "k = 0"
    got = run_host(dlaf, grid, t, "N", "N", alpha, ak, bk, dt(0), nan, nb)
    assert np.array_equal(got, np.zeros_like(c0)), "k = 0, beta = 0 over NaN"
    # m = 0 and n = 0 return
    for mm, nn in ((0, n), (m, 0)):
        a0, b0, ce = (np.zeros(s, dtype=dt, order="F") for s in ((mm, k), (k, nn), (mm, nn)))
        dlaf.general_multiplication(grid, "N", "N", alpha, a0, b0, beta, ce, nb)
    # beta = 1, alpha = -1
    got = run_host(dlaf, grid, t, "N", "N", dt(-1), a, b, dt(1), c0, nb)
    assert np.array_equal(got, reference(t, "N", "N", -1, a, b, 1, c0).astype(dt)), "beta = 1, alpha = -1"


@pytest.mark.parametrize("t", ["c", "z"])
def test_transpose_and_adjoint_differ(dlaf, grid, t):
    """T and C on the same operand give different results, each its own reference's"""
    m, n, k, nb = 70, 50, 60, 32
    alpha, beta = scalars(t)
    for which in (0, 1):
        res = {}
        for o in "TC":
            opa, opb = (o, "N") if which == 0 else ("N", o)
            a, b, c0 = operands(integers, np.random.default_rng(36), t, opa, opb, m, n, k)  # the same operands for T and C
            res[o] = run_host(dlaf, grid, t, opa, opb, alpha, a, b, beta, c0, nb)
            assert np.array_equal(res[o], reference(t, opa, opb, alpha, a, b, beta, c0).astype(DT[t])), (which, o)
        assert not np.array_equal(res["T"], res["C"]), which


@pytest.mark.parametrize("t", TYPES)
def test_uniform_random_operands(dlaf, grid, t):
    """Component-wise bound of an inner product in ANY summation order (Higham, Accuracy and Stability of Numerical
    Algorithms, 2nd ed., section 3.1): fl(sum_k a_k b_k) differs from the sum by at most gamma_k sum |a_k||b_k| with
    gamma_k = k u / (1 - k u); the product with alpha, the product beta c and the final sum add three more roundings to
    the first term and two to the second, so  |C - C^| <= (k + 4) u (|alpha| |A| |B| + |beta| |C0|)  to first order in
    u, u the unit roundoff of the type.  A complex product or sum computed from real operations carries a constant
    below 2 sqrt(2) per operation instead of 1 (ibid. section 3.6) and the moduli bound the parts: the factor 4.  The
    reference is computed in the wider type (its own error is below u^2 here)."""
    rng = np.random.default_rng(37)
    m, n, k = SHAPE
    dt, w = DT[t], WIDE[t]
    alpha = dt(complex(-1.2, .7)) if t in "cz" else dt(-1.2)
    beta = dt(complex(1.12, -.1)) if t in "cz" else dt(1.12)
    for opa, opb in (("N", "N"), ("C", "T")):
        a, b, c0 = operands(uniform, rng, t, opa, opb, m, n, k)
        got = run_host(dlaf, grid, t, opa, opb, alpha, a, b, beta, c0, 160)
        want = reference(t, opa, opb, alpha, a, b, beta, c0)
        u = float(np.finfo(dt).eps) / 2
        real_w = np.longdouble if w in (np.longdouble, np.clongdouble) else np.float64
        mag = abs(w(alpha)) * (np.abs(op_of(a, opa)).astype(real_w) @ np.abs(op_of(b, opb)).astype(real_w)) + \
            abs(w(beta)) * np.abs(c0).astype(real_w)
        bound = (4 if t in "cz" else 1) * (k + 4) * u * mag
        err = np.abs(got.astype(w) - want)
        print(f"uniform {t} {opa}{opb}: max err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (t, opa, opb, float((err / bound).max()))


@pytest.mark.parametrize("opa,opb", [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")])
@pytest.mark.parametrize("t", ["d", "z"])
def test_resident(dlaf, grid, t, opa, opb):
    """three GeneralDeviceMatrix operands: only C changes"""
    rng = np.random.default_rng(38)
    m, n, k, nb = 357, 165, 192, 160
    dt = DT[t]
    alpha, beta = scalars(t)
    a, b, c0 = operands(integers, rng, t, opa, opb, m, n, k)
    A = dlaf.GeneralDeviceMatrix(grid, dt, a.shape[0], a.shape[1], nb)
    B = dlaf.GeneralDeviceMatrix(grid, dt, b.shape[0], b.shape[1], nb)
    Cm = dlaf.GeneralDeviceMatrix(grid, dt, m, n, nb)
    A.upload(a)
    B.upload(b)
    Cm.upload(c0)
    dlaf.general_multiplication_device(opa, opb, alpha, A, B, beta, Cm)
    got, fa, fb = (np.zeros(x.shape, dtype=dt, order="F") for x in (c0, a, b))
    Cm.download(got)
    A.download(fa)
    B.download(fb)
    assert np.array_equal(got, reference(t, opa, opb, alpha, a, b, beta, c0).astype(dt)), (t, opa, opb)
    assert np.array_equal(fa, a) and np.array_equal(fb, b), "A or B changed"
    ms, flops = dlaf.multiplication_profile()
    assert ms > 0 and flops == (8 if t == "z" else 2) * m * n * k, (ms, flops)
    for h in (Cm, B, A):
        h.close()


@pytest.mark.parametrize("t", ["d", "z"])
def test_pxgemm(dlaf, grid, t):
    """p?gemm with 9-int descriptors on a 1 x 1 grid"""
    rng = np.random.default_rng(39)
    alpha, beta = scalars(t)
    for (m, n, k, nb), (opa, opb) in itertools.product([(150, 70, 90, 32), (64, 200, 130, 64)], [("N", "N"), ("C", "T")]):
        a, b, c0 = operands(integers, rng, t, opa, opb, m, n, k)
        c = c0.copy(order="F")
        dlaf.pxgemm(opa, opb, m, n, k, alpha, a, 1, 1, [1, grid.context, a.shape[0], a.shape[1], nb, nb, 0, 0, a.shape[0]],
                    b, 1, 1, [1, grid.context, b.shape[0], b.shape[1], nb, nb, 0, 0, b.shape[0]], beta,
                    c, 1, 1, [1, grid.context, m, n, nb, nb, 0, 0, m])
        assert np.array_equal(c, reference(t, opa, opb, alpha, a, b, beta, c0).astype(DT[t])), (t, m, n, k, opa, opb)
