"""general_addition on the GPU: C = beta C + alpha op(A) on the uplo part, every op x uplo x type on one process, through
the host entry (padded arrays) and the resident one, against numpy.

Exact operands: integer entries in [-3, 3] (complex: both parts), alpha = 2 - 1j and beta = -1 + 2j (2 and -3 for real
types): every product and sum is an integer far below 2^24, exact in all four types, so the tests assert equality.

The kernel cuts a tile into B x B sub-blocks, B = 64 for s / d / c and 32 for z, and moves 16 bytes per access where the
tile columns are 16-byte aligned.  The shapes (nb, m, n) are the smallest that reach every path of it:
  (160, 357, 165)  several sub-blocks per tile with a ragged one (160 = 2 * 64 + 32 = 5 * 32: z has no ragged one here,
                   it has at nb = 48), ragged last tiles on both dimensions, 3 x 2 tiles so that T is not square
  (48, 100, 75)    a single ragged sub-block for B = 64; two sub-blocks, one ragged, for B = 32
  (24, 50, 31)     a single ragged sub-block for B = 32
  (33, 70, 40)     no 16-byte alignment anywhere for s, d, c: the element path
  (50, 60, 110)    the element path for s (200-byte columns), the 16-byte one for d, c, z
  (64, 64, 64)     one tile, m = n = nb
  (32, 1, 45), (32, 45, 1)   a single row, a single column
Outside the uplo part C is NaN on entry and must come back bit for bit, like the padding rows of its leading dimension
and all of A, padding included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TYPES = ["s", "d", "c", "z"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
WIDE = {"s": np.float64, "d": np.longdouble, "c": np.complex128, "z": np.clongdouble}
UNIT = {"s": 2.0 ** -24, "d": 2.0 ** -53, "c": 2.0 ** -24, "z": 2.0 ** -53}
SHAPES = [(160, 357, 165), (48, 100, 75), (24, 50, 31), (33, 70, 40), (50, 60, 110), (64, 64, 64), (32, 1, 45), (32, 45, 1)]
OPS = ["N", "T", "C"]
UPLOS = ["A", "L", "U"]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def fortran(x, dtype=None):
    """a column-major copy whose first stride is the item size also for a single row"""
    out = np.empty(x.shape, dtype=dtype or x.dtype, order="F")
    out[...] = x
    return out


def scalars(t):
    return (DT[t](2 - 1j), DT[t](-1 + 2j)) if t in "cz" else (DT[t](2), DT[t](-3))


def integers(rng, t, shape):
    x = rng.integers(-3, 4, shape).astype(np.float64)
    if t in "cz":
        x = x + 1j * rng.integers(-3, 4, shape)
    return fortran(x, DT[t])


def uniform(rng, t, shape):
    x = rng.uniform(-1, 1, shape)
    if t in "cz":
        x = x + 1j * rng.uniform(-1, 1, shape)
    return fortran(x, DT[t])


def in_part(uplo, m, n):
    i, j = np.indices((m, n))
    return np.ones((m, n), bool) if uplo == "A" else (i >= j if uplo == "L" else i <= j)


def op_of(op, a):
    return a if op == "N" else (a.T if op == "T" else a.conj().T)


def padded(x, extra, fill):
    store = np.full((x.shape[0] + extra, max(1, x.shape[1])), fill, dtype=x.dtype, order="F")
    view = store[:x.shape[0], :x.shape[1]]
    view[...] = x
    return store, view


def run_host(dlaf, grid, uplo, op, alpha, a, beta, c_in, nb):
    """the host entry on padded arrays; asserts that A, the padding of C and C outside the part kept their bits"""
    m, n = c_in.shape
    part = in_part(uplo, m, n)
    sa, va = padded(a, 3, np.nan)
    sc, vc = padded(c_in, 5, np.nan)
    before_a, pad_c, other = sa.tobytes(), sc[m:, :].tobytes(), vc[~part].tobytes()
    dlaf.general_addition(grid, uplo, op, alpha, va, beta, vc, nb, m=m, n=n)
    assert sa.tobytes() == before_a, "A (padding included) changed"
    assert sc[m:, :].tobytes() == pad_c, "the padding rows of C changed"
    assert vc[~part].tobytes() == other, "C outside the uplo part changed"
    return fortran(vc)


def run_device(dlaf, grid, t, uplo, op, alpha, a, beta, c_in, nb):
    """the resident entry; asserts that A and C outside the part kept their bits"""
    m, n = c_in.shape
    part = in_part(uplo, m, n)
    ga = dlaf.GeneralDeviceMatrix(grid, DT[t], a.shape[0], a.shape[1], nb)
    gc = dlaf.GeneralDeviceMatrix(grid, DT[t], m, n, nb)
    ga.upload(a)
    gc.upload(c_in)
    dlaf.general_addition_device(uplo, op, alpha, ga, beta, gc)
    out, a_back = fortran(np.zeros_like(c_in)), fortran(np.zeros_like(a))
    gc.download(out)
    ga.download(a_back)
    ga.close()
    gc.close()
    assert a_back.tobytes() == a.tobytes(), "the resident A changed"
    assert out[~part].tobytes() == c_in[~part].tobytes(), "the resident C outside the uplo part changed"
    return out


def both(dlaf, grid, t, uplo, op, alpha, a, beta, c_in, nb):
    return {"host": run_host(dlaf, grid, uplo, op, alpha, a, beta, c_in, nb),
            "resident": run_device(dlaf, grid, t, uplo, op, alpha, a, beta, c_in, nb)}


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", UPLOS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("nb,m,n", SHAPES)
def test_exact(dlaf, grid, nb, m, n, op, uplo, t):
    rng = np.random.default_rng(7 * nb + m + 3 * n)
    alpha, beta = scalars(t)
    a = integers(rng, t, (m, n) if op == "N" else (n, m))
    c0 = integers(rng, t, (m, n))
    part = in_part(uplo, m, n)
    c_in = fortran(np.where(part, c0, np.nan), DT[t])
    want = (beta * c0 + alpha * op_of(op, a)).astype(DT[t])
    for how, got in both(dlaf, grid, t, uplo, op, alpha, a, beta, c_in, nb).items():
        assert np.array_equal(got[part], want[part]), (how, np.argwhere((got != want) & part)[:5])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", ["A", "L"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("nb,m,n", [(160, 357, 165), (33, 70, 40)])
def test_beta_zero_does_not_read_c_and_alpha_zero_does_not_reference_a(dlaf, grid, nb, m, n, op, uplo, t):
    rng = np.random.default_rng(11)
    alpha, beta = scalars(t)
    a = integers(rng, t, (m, n) if op == "N" else (n, m))
    c0 = integers(rng, t, (m, n))
    part = in_part(uplo, m, n)
    nan_c = np.full((m, n), np.nan, dtype=DT[t], order="F")
    want = (alpha * op_of(op, a)).astype(DT[t])
    for how, got in both(dlaf, grid, t, uplo, op, alpha, a, 0, nan_c, nb).items():
        assert not np.isnan(got[part]).any(), how
        assert np.array_equal(got[part], want[part]), how
    nan_a = fortran(np.full_like(a, np.nan))
    c_in = fortran(np.where(part, c0, np.nan), DT[t])
    want = (beta * c0).astype(DT[t])
    for how, got in both(dlaf, grid, t, uplo, op, 0, nan_a, beta, c_in, nb).items():
        assert not np.isnan(got[part]).any(), how
        assert np.array_equal(got[part], want[part]), how
    # alpha = 0 and beta = 0: exact zeros, whatever both held
    for how, got in both(dlaf, grid, t, uplo, op, 0, nan_a, 0, nan_c, nb).items():
        assert np.array_equal(got[part], np.zeros((m, n), DT[t])[part]), how


def special_values(rng, t, shape):
    """doubles that a multiplication by 1 or an addition of 0 would change or that compare unequal to themselves: -0.0,
    +-Inf, denormals, quiet and signalling NaNs with distinct payloads"""
    def plane():
        bits = rng.integers(0x3ff0000000000000, 0x4000000000000000, shape, dtype=np.uint64)
        k = np.arange(bits.size, dtype=np.uint64).reshape(shape)
        kind = rng.integers(0, 12, shape)
        bits = np.where(kind == 0, np.uint64(0x8000000000000000), bits)
        bits = np.where(kind == 1, np.uint64(0x7ff0000000000000), bits)
        bits = np.where(kind == 2, np.uint64(0xfff0000000000000), bits)
        bits = np.where(kind == 3, np.uint64(1) + k, bits)                         # denormals
        bits = np.where(kind == 4, np.uint64(0x800fffffffffffff) - k, bits)        # negative denormals
        bits = np.where(kind == 5, np.uint64(0x7ff8000000000001) + k, bits)        # quiet NaNs
        bits = np.where(kind == 6, np.uint64(0xfff0000000000001) + k, bits)        # signalling NaNs
        return fortran(bits, np.uint64)
    if t == "d":
        return plane().view(np.float64)
    z = np.zeros(shape, dtype=np.complex128, order="F")
    z.real = plane().view(np.float64)
    z.imag = plane().view(np.float64)
    return z


@pytest.mark.parametrize("t", ["d", "z"])
@pytest.mark.parametrize("op", ["N", "T"])
@pytest.mark.parametrize("uplo", UPLOS)
@pytest.mark.parametrize("nb,m,n", [(160, 357, 165), (33, 70, 40)])
def test_alpha_one_beta_zero_is_a_bit_copy(dlaf, grid, nb, m, n, uplo, op, t):
    rng = np.random.default_rng(5)
    a = special_values(rng, t, (m, n) if op == "N" else (n, m))
    part = in_part(uplo, m, n)
    c_in = special_values(rng, t, (m, n))
    want = fortran(a if op == "N" else a.T)
    with np.errstate(all="ignore"):
        assert want[part].tobytes() != (want[part] * 1 + 0).tobytes(), "the operand would survive a multiply-add"
    for how, got in both(dlaf, grid, t, uplo, op, 1, a, 0, c_in, nb).items():
        assert got[part].tobytes() == want[part].tobytes(), how


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", UPLOS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("nb,m,n", [(160, 357, 165), (33, 70, 40)])
def test_uniform_operands_within_the_rounding_bound(dlaf, grid, nb, m, n, op, uplo, t):
    """|got - want| <= c u (|beta| |C| + |alpha| |A|) component-wise, c = 3 (real) / 6 (complex): a multiply-add, fused
    or not, is below 2 u, a complex product below sqrt(5) u, each addition adds one u.  No entry is left out."""
    rng = np.random.default_rng(13)
    w = WIDE[t]
    alpha = DT[t](0.7 - 0.4j) if t in "cz" else DT[t](0.7)
    beta = DT[t](-0.3 + 0.9j) if t in "cz" else DT[t](-1.3)
    a = uniform(rng, t, (m, n) if op == "N" else (n, m))
    c0 = uniform(rng, t, (m, n))
    part = in_part(uplo, m, n)
    want = w(beta) * c0.astype(w) + w(alpha) * op_of(op, a).astype(w)
    bound = (6 if t in "cz" else 3) * UNIT[t] * (abs(w(beta)) * np.abs(c0.astype(w)) + abs(w(alpha)) * np.abs(op_of(op, a).astype(w)))
    for how, got in both(dlaf, grid, t, uplo, op, alpha, a, beta, c0, nb).items():
        diff = got.astype(w) - want
        worst = np.maximum(np.abs(diff.real), np.abs(diff.imag))
        ratio = float(np.max(np.where(part, worst / bound, 0)))
        print(f"{how} {t} {op} {uplo} nb {nb}: worst error / bound = {ratio:.3f}")
        assert np.all(worst[part] <= bound[part]), (how, ratio)
        assert got[~part].tobytes() == c0[~part].tobytes(), how


@pytest.mark.parametrize("t", TYPES)
def test_op_n_in_place(dlaf, grid, t):
    """A and C the same array / handle with op N: C = (alpha + beta) C on the part"""
    nb, m, n = 48, 100, 75
    rng = np.random.default_rng(3)
    alpha, beta = scalars(t)
    c0 = integers(rng, t, (m, n))
    part = in_part("L", m, n)
    want = ((alpha + beta) * c0).astype(DT[t])
    c = c0.copy(order="F")
    dlaf.general_addition(grid, "L", "N", alpha, c, beta, c, nb)
    assert np.array_equal(c[part], want[part]) and c[~part].tobytes() == c0[~part].tobytes()
    g = dlaf.GeneralDeviceMatrix(grid, DT[t], m, n, nb)
    g.upload(c0)
    dlaf.general_addition_device("L", "N", alpha, g, beta, g)
    out = np.zeros_like(c0)
    g.download(out)
    g.close()
    assert np.array_equal(out[part], want[part]) and out[~part].tobytes() == c0[~part].tobytes()


def desc9(grid, m, n, nb, ld):
    return [1, grid.context, m, n, nb, nb, 0, 0, ld]


@pytest.mark.parametrize("t", ["d", "z"])
def test_scalapack_entries_give_the_native_bits(dlaf, grid, t):
    nb, m, n = 48, 100, 75
    rng = np.random.default_rng(17)
    alpha, beta = scalars(t)
    a_n, a_t, c0 = uniform(rng, t, (m, n)), uniform(rng, t, (n, m)), uniform(rng, t, (m, n))
    dn, dt, dc = desc9(grid, m, n, nb, m), desc9(grid, n, m, nb, n), desc9(grid, m, n, nb, m)

    def native(uplo, op, al, a, be):
        c = c0.copy(order="F")
        dlaf.general_addition(grid, uplo, op, al, a, be, c, nb)
        return c

    c = c0.copy(order="F")
    dlaf.pxgeadd("N", m, n, alpha, a_n, 1, 1, dn, beta, c, 1, 1, dc)
    assert c.tobytes() == native("A", "N", alpha, a_n, beta).tobytes()
    c = c0.copy(order="F")
    dlaf.pxgeadd("C", m, n, alpha, a_t, 1, 1, dt, beta, c, 1, 1, dc)
    assert c.tobytes() == native("A", "C", alpha, a_t, beta).tobytes()
    c = c0.copy(order="F")
    dlaf.pxtradd("U", "T", m, n, alpha, a_t, 1, 1, dt, beta, c, 1, 1, dc)
    assert c.tobytes() == native("U", "T", alpha, a_t, beta).tobytes()
    c = c0.copy(order="F")
    dlaf.pxtran(m, n, alpha, a_t, 1, 1, dt, beta, c, 1, 1, dc)
    assert c.tobytes() == native("A", "T", alpha, a_t, beta).tobytes()
    if t == "z":
        c = c0.copy(order="F")
        dlaf.pxtran(m, n, alpha, a_t, 1, 1, dt, beta, c, 1, 1, dc, conj=True)
        assert c.tobytes() == native("A", "C", alpha, a_t, beta).tobytes()
    for uplo, part in (("L", "L"), ("U", "U"), ("G", "A")):
        c = c0.copy(order="F")
        dlaf.pxlacpy(uplo, m, n, a_n, 1, 1, dn, c, 1, 1, dc)
        assert c.tobytes() == native(part, "N", 1, a_n, 0).tobytes()
        assert c[in_part(part, m, n)].tobytes() == a_n[in_part(part, m, n)].tobytes()


def test_resident_refusals(dlaf, grid):
    """what only a resident call can get wrong is refused in a child process: the parent keeps its GPU state"""
    import subprocess
    import sys
    code = ("import numpy as np, dla_future_amd as d\n"
            "d.initialize(); g = d.Grid.single()\n"
            "a = d.GeneralDeviceMatrix(g, np.float64, 6, 4, 2); c = d.GeneralDeviceMatrix(g, np.float64, 6, 6, 2)\n"
            "d.general_addition_device('A', 'T', 1.0, c, 0.0, c)\nprint('survived')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "survived" not in r.stdout
    assert "general addition: A and C are the same matrix, which only op 'N' accepts" in r.stderr, r.stderr[-500:]
